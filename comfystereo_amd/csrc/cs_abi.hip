// cs_abi.hip -- the extern "C" boundary (include/comfystereo_amd.h) and the small streaming kernels
// around the row kernels: depth grayscale + per-frame min/max, bilinear depth resize, per-frame
// decisions (0..255 scaling), device self-tests of the libm-exact math.
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <vector>

#include "cs_common.h"
#include "cs_kernels.h"
#include "cs_latent.h"
#include "cs_motiondepth.h"
#include "cs_motionpyramid.h"

namespace cs {

static thread_local char g_err[256] = "";
static int fail(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}
static int fail_hip(hipError_t e, const char* where) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return CS_EHIP;
}

// launch_blur's three failure classes get their own message (CS_EHIP reads the HIP error that caused it)
static int fail_blur(int rc) {
    if (rc == CS_EHIP) return fail_hip(hipGetLastError(), "depth blur");
    if (rc == CS_ELIMIT) return fail(rc, "depth blur: frame or blur kernel too wide for the LDS of the two-pass path");
    return fail(rc, "depth blur: unsupported parameters (strength must round to >= 1)");
}

// development switches: explicit state set through cs_debug_set (never the environment)
static std::atomic<int> g_dev[CS_DEBUG_KEYS];
int dev_switch(int key) { return (key >= 0 && key < CS_DEBUG_KEYS) ? g_dev[key].load(std::memory_order_relaxed) : 0; }

// the classes of techniques, modes and parameters the host code below asks about
static bool is_poly(int fill) { return fill == CS_FILL_POLYLINES_SOFT || fill == CS_FILL_POLYLINES_SHARP; }
static bool is_hybrid(int fill) { return fill == CS_FILL_HYBRID_EDGE || fill == CS_FILL_HYBRID_EDGE_PLUS; }
static bool is_anaglyph(int mode) { return mode == CS_MODE_RED_CYAN_ANAGLYPH || mode == CS_MODE_CYAN_RED_REVERSEANAGLYPH; }
static bool blur_on(const cs_params* p) { return p->depth_map_blur && p->depth_blur_strength > 0; }   // (<= 0: the reference returns the depth as is, :1194, :1050)
// gpu_warp: the frames of one reference sub-batch (they share the x255 decision, :1045)
static int warp_group(const cs_params* p) { return p->batch_size > 0 ? (p->batch_size < p->n ? p->batch_size : p->n) : p->n; }

// ---------------------------------------------------------------------------------------------
// streaming kernels
// ---------------------------------------------------------------------------------------------
__global__ void k_stats_init(uint32_t* stats, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * ST_WORDS) return;
    int wd = i % ST_WORDS;
    bool is_min = wd == ST_GRAY_MIN || wd == ST_L_MIN || wd == ST_R_MIN;
    stats[i] = is_min ? 0xffffffffu : 0u;
}

__device__ __forceinline__ void block_minmax_commit(float mn, float mx, uint32_t* st_min, uint32_t* st_max) {
    __shared__ float red[2 * 16];
    block_minmax_update(mn, mx, st_min, st_max, red);
}

// gray = (0.2989 R + 0.5870 G) + 0.1140 B with separate float32 roundings (GenerateStereo.py:134-139,
// 206-209); C == 1 -> the channel; other C -> channel 0.  grid: (blocks, n).
__global__ void __launch_bounds__(256) k_gray(const float* __restrict__ depth, float* __restrict__ gray, int hw,
                                              int c, uint32_t* stats, int do_minmax) {
    const int frame = blockIdx.y;
    const float* src = depth + (size_t)frame * hw * c;
    float* dst = gray + (size_t)frame * hw;
    float mn = INFINITY, mx = -INFINITY;
    const int stride = gridDim.x * blockDim.x;
    if (c == 3 && (hw & 3) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < hw / 4; q += stride) {
            float4 a = s4[3 * q], b = s4[3 * q + 1], cc = s4[3 * q + 2];
            float4 g;
            g.x = gray_of(a.x, a.y, a.z);
            g.y = gray_of(a.w, b.x, b.y);
            g.z = gray_of(b.z, b.w, cc.x);
            g.w = gray_of(cc.y, cc.z, cc.w);
            d4[q] = g;
            mn = fminf(fminf(mn, g.x), fminf(g.y, fminf(g.z, g.w)));
            mx = fmaxf(fmaxf(mx, g.x), fmaxf(g.y, fmaxf(g.z, g.w)));
        }
    } else {
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += stride) {
            float g;
            if (c == 3) g = gray_of(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
            else g = src[(size_t)i * c];
            dst[i] = g;
            mn = fminf(mn, g);
            mx = fmaxf(mx, g);
        }
    }
    if (do_minmax) block_minmax_commit(mn, mx, &stats[frame * ST_WORDS + ST_GRAY_MIN], &stats[frame * ST_WORDS + ST_GRAY_MAX]);
}

// per-frame min/max of a [n][hw] float array into the given stats words.  fminf / fmaxf drop a NaN.  NAN_POISONS (the latent
// shifts only): a NaN anywhere makes the max word a NaN, as torch's min() / max() return one (reference stereo_utils.py:38-40) --
// the key of a positive NaN lies above +inf's, so the atomic max keeps it; the range is then no number and the map counts as flat.
template <bool NAN_POISONS>
__global__ void __launch_bounds__(256) k_minmax(const float* __restrict__ a, int hw, uint32_t* stats, int wmin, int wmax) {
    const int frame = blockIdx.y;
    const float* src = a + (size_t)frame * hw;
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
        float g = src[i];
        mn = fminf(mn, g);
        mx = fmaxf(mx, g);
        if (NAN_POISONS) nan |= g != g;
    }
    block_minmax_commit(mn, mx, &stats[frame * ST_WORDS + wmin], &stats[frame * ST_WORDS + wmax]);
    if (NAN_POISONS) {
        if (__syncthreads_or(nan) && threadIdx.x == 0) atomicMax(&stats[frame * ST_WORDS + wmax], csm::f2ord(csm::u2f(0x7fc00000u)));
    }
}

// F.interpolate(mode='bilinear', align_corners=False) of the gray depth (GenerateStereo.py:141-148, 214-220) + min/max of the
// result, bit for bit as CPU torch 2.10 computes it (probed against torch in the build container, tests/golden/resize.npz):
//   source index = fma(scale, dst + 0.5, -0.5) clamped at 0 (scale = (float)in / out; the compiler contracts the expression),
//   lambda1 = index - floor, lambda0 = 1 - lambda1, second tap = first + 1 unless at the border;
//   outputs with out_h + out_w > 128 take the separable loop  fma(t0, wy0, t1 * wy1), t = fma(a, wx0, b * wx1);
//   smaller ones the four-tap loop over weight products  fma(d, wy1*wx1, fma(c, wy1*wx0, fma(a, wy0*wx0, b * (wy0*wx1))))
//   (which of its two loops torch's TensorIterator picks depends on out_h + out_w only: scanned for 3 <= out_h <= 300 and every
//   out_w up to 4200 pixels per frame, independent of the input size, the batch and the thread count).
__global__ void __launch_bounds__(256) k_resize_bilinear(const float* __restrict__ in, int ih, int iw,
                                                         float* __restrict__ out, int oh, int ow, uint32_t* stats) {
    const int frame = blockIdx.y;
    const float* src = in + (size_t)frame * ih * iw;
    float* dst = out + (size_t)frame * oh * ow;
    const float sy = (float)ih / (float)oh, sx = (float)iw / (float)ow;
    const bool small = oh + ow <= 128;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < oh * ow; i += gridDim.x * blockDim.x) {
        const int y = i / ow, x = i - y * ow;
        const float fy = fmaxf(fmaf(sy, (float)y + 0.5f, -0.5f), 0.0f), fx = fmaxf(fmaf(sx, (float)x + 0.5f, -0.5f), 0.0f);
        const int y0 = min((int)fy, ih - 1), x0 = min((int)fx, iw - 1);
        const int y1 = y0 + (y0 < ih - 1 ? 1 : 0), x1 = x0 + (x0 < iw - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float hy = 1.0f - ly, hx = 1.0f - lx;
        const float a = src[y0 * iw + x0], b = src[y0 * iw + x1], c = src[y1 * iw + x0], d = src[y1 * iw + x1];
        float v;
        if (small) {
            v = b * (hy * lx);
            v = fmaf(a, hy * hx, v);
            v = fmaf(c, ly * hx, v);
            v = fmaf(d, ly * lx, v);
        } else {
            const float t0 = fmaf(a, hx, b * lx), t1 = fmaf(c, hx, d * lx);
            v = fmaf(t0, hy, t1 * ly);
        }
        dst[i] = v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    block_minmax_commit(mn, mx, &stats[frame * ST_WORDS + ST_GRAY_MIN], &stats[frame * ST_WORDS + ST_GRAY_MAX]);
}

// per-frame decisions that the reference takes on host scalars (kept on device: no sync)
//   CPU techniques: `if depthmap.max() <= 1.0: depthmap *= 255`, per frame (:1475)
//   gpu_warp:       `if depth_tensor.amax() <= 1.0` over the sub-batch (:1045)
__global__ void k_finalize_stats(uint32_t* stats, int n, int group, int blur) {
    int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    float gmax = csm::ord2f(stats[f * ST_WORDS + ST_GRAY_MAX]);
    float gmin = csm::ord2f(stats[f * ST_WORDS + ST_GRAY_MIN]);
    float dec = gmax;
    if (group > 0) {
        int g0 = (f / group) * group, g1 = min(g0 + group, n);
        for (int k = g0; k < g1; k++) dec = fmaxf(dec, csm::ord2f(stats[k * ST_WORDS + ST_GRAY_MAX]));
    }
    uint32_t sc = dec <= 1.0f ? 1u : 0u;
    stats[f * ST_WORDS + ST_SCALE255] = sc;
    if (!blur) {
        float s = sc ? 255.0f : 1.0f;
        uint32_t mn = csm::f2ord(gmin * s), mx = csm::f2ord(gmax * s);
        stats[f * ST_WORDS + ST_L_MIN] = mn;
        stats[f * ST_WORDS + ST_R_MIN] = mn;
        stats[f * ST_WORDS + ST_L_MAX] = mx;
        stats[f * ST_WORDS + ST_R_MAX] = mx;
    }
}

// uint8 codes -> float32 k/255 (true division through a LUT), 4 values per thread
__global__ void __launch_bounds__(256) k_expand_u8(const uint8_t* __restrict__ in, float* __restrict__ out, size_t count) {
    __shared__ float lut[256];
    lut[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    const size_t nq = count / 4, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nq; i += stride) {
        uint32_t pk = reinterpret_cast<const uint32_t*>(in)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(lut[pk & 0xff], lut[(pk >> 8) & 0xff], lut[(pk >> 16) & 0xff], lut[pk >> 24]);
    }
    for (size_t i = 4 * nq + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += stride) out[i] = lut[in[i]];
}


// float32 node outputs -> their uint8 codes (the compact form the host pipeline moves over PCIe): mode 0: value k / 255 -> k
// (exact: fl(k / 255) * 255 lies within half an ulp-scale of k); mode 1: non-zero flag (mask).  `stride` floats between
// consecutive values (3: one code per pixel of a three-equal-channel depth map).
__global__ void __launch_bounds__(256) k_pack_u8(const float* __restrict__ in, uint8_t* __restrict__ out, size_t count, int stride,
                                                 int mode) {
    const size_t nq = count / 4, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nq; i += step) {
        uint32_t pk = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float v = in[(4 * i + j) * (size_t)stride];
            const uint32_t k = mode ? (v != 0.0f ? 1u : 0u) : (uint32_t)__builtin_rintf(v * 255.0f);
            pk |= (k & 0xffu) << (8 * j);
        }
        reinterpret_cast<uint32_t*>(out)[i] = pk;
    }
    for (size_t i = 4 * nq + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += step) {
        const float v = in[i * (size_t)stride];
        out[i] = (uint8_t)(mode ? (v != 0.0f ? 1u : 0u) : (uint32_t)__builtin_rintf(v * 255.0f));
    }
}

// every stride-th float (one channel of a depth-map output with equal channels)
__global__ void __launch_bounds__(256) k_take_f32(const float* __restrict__ in, float* __restrict__ out, size_t count, int stride) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += step) out[i] = in[i * (size_t)stride];
}

// ---------------------------------------------------------------------------------------------
// stereo_shift_torch (reference stereo_utils.py:15-88): the `none` forward map on a float payload (latents [b][c][h][w]).
// One workgroup per (row, batch item): winner source column per destination by LDS atomics (the reference's sweep makes the
// largest source column win for a negative shift and the smallest for a positive one, :56-67), then a gather of all channels.
// The depth is normalised with the GLOBAL min / max of the whole depth tensor (:36-45), unfilled destinations stay 0.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_stereo_shift(const float* __restrict__ in, const float* __restrict__ depth, int c, int h,
                                                      int w, const uint32_t* stats, float scale_px32, int asc, int pow_mode,
                                                      float e32, float* __restrict__ out) {
    extern __shared__ int win[];   // [w] winning source column per destination, -1 = none
    __shared__ csm::PowfTables T;
    const int row = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) { const csm::PowfTables init = CS_POWF_TABLES_INIT; T = init; }
    for (int x = tid; x < w; x += blockDim.x) win[x] = asc ? -1 : 0x7fffffff;
    __syncthreads();
    const float mn = csm::ord2f(stats[ST_L_MIN]), mx = csm::ord2f(stats[ST_L_MAX]);
    const float rng = mx - mn;
    const bool flat = !(rng > 1.1920929e-07f);   // torch.finfo(float32).eps (:40)
    const float* drow = depth + ((size_t)b * h + row) * w;
    for (int col = tid; col < w; col += blockDim.x) {
        int cd;
        if (stereo_shift_dest(drow[col], mn, rng, flat, pow_mode, e32, scale_px32, col, w, &T, cd)) {
            if (asc) atomicMax(&win[cd], col);
            else atomicMin(&win[cd], col);
        }
    }
    __syncthreads();
    for (int i = tid; i < c * w; i += blockDim.x) {
        const int ch = i / w, x = i - ch * w;
        const int src = win[x];
        const size_t base = (((size_t)b * c + ch) * h + row) * w;
        out[base + x] = (src >= 0 && src < w) ? in[base + src] : 0.0f;
    }
}

__global__ void k_test_powf(const float* x, float y, float* out, size_t n) {
    __shared__ csm::PowfTables T;
    const csm::PowfTables init = CS_POWF_TABLES_INIT;
    if (threadIdx.x == 0) T = init;
    __syncthreads();
    // both forms: the SIMT-shaped one the kernels use must equal the plain one bit for bit
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float a = csm::powf_exact(x[i], y, &T), b = csm::powf_exact_simt(x[i], y, &T);
        out[i] = csm::f2u(a) == csm::f2u(b) ? a : csm::u2f(0x7fc00001u);
        // the exponent shortcuts of the tile kernel (x >= 0 only, like |nd|) must agree as well
        if (x[i] >= 0.0f && y == 1.0f && csm::f2u(x[i]) != csm::f2u(a)) out[i] = csm::u2f(0x7fc00002u);
        if (x[i] >= 0.0f && y == 2.0f) {
            bool risky;
            const float sq = csm::square_or_flag(x[i], risky);
            if (!risky && csm::f2u(sq) != csm::f2u(a)) out[i] = csm::u2f(0x7fc00003u);
        }
    }
}

__device__ const unsigned long long d_exp_tab[256] = {CS_EXP_TAB_VALUES};

__global__ void k_test_exp(const double* x, double* out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = csm::exp_exact(x[i], d_exp_tab);
}

// ---- measurement hook (cs_profile / cs_profile_read) ------------------------------------------
// The event pool is process-wide opt-in state (cs_profile); every access holds g_prof_mu, so concurrent cs_generate
// calls on different streams / threads may record into it.
static const int PROF_MAX = 4096;
static std::mutex g_prof_mu;
static std::atomic<bool> g_prof_on{false};
static hipEvent_t g_prof_ev[2 * PROF_MAX];
static int g_prof_made = 0, g_prof_used = 0;
// the lazy-tile map of the last profiled cs_generate call (null: the call's warp kernel read complete blurred maps)
// share of the lazy blur tiles the profiled calls wrote (cs_profile_tiles): counted on the device into a LIBRARY-OWNED pair of
// words {tiles set, tiles in all}, accumulated over the chunks of every profiled cs_generate -- no pointer into a caller's
// workspace outlives the call
static unsigned long long* g_prof_tiles = nullptr;
static bool g_prof_tiles_any = false;
static hipStream_t g_prof_tiles_stream = nullptr;
__global__ void __launch_bounds__(256) k_prof_count_tiles(const uint32_t* __restrict__ map, int rows, int words, int tcols,
                                                          unsigned long long* acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned cnt = 0;
    if (i < rows * words) {
        const int wi = i % words, first = wi * 32;
        const int valid = tcols - first;   // tiles of the row this word holds (the pad word and the tail bits: none)
        const uint32_t m = valid >= 32 ? 0xffffffffu : (valid <= 0 ? 0u : (1u << valid) - 1u);
        cnt = __popc(map[i] & m);
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&acc[0], (unsigned long long)cnt);
    if (i == 0) atomicAdd(&acc[1], (unsigned long long)rows * (unsigned long long)tcols);
}
struct ProfScope {
    hipStream_t s; int slot;
    explicit ProfScope(hipStream_t stream) : s(stream), slot(-1) {
        if (!g_prof_on.load(std::memory_order_relaxed)) return;
        std::lock_guard<std::mutex> lock(g_prof_mu);
        if (g_prof_used >= PROF_MAX) return;
        while (g_prof_made <= g_prof_used) {
            if (hipEventCreate(&g_prof_ev[2 * g_prof_made]) != hipSuccess) return;
            if (hipEventCreate(&g_prof_ev[2 * g_prof_made + 1]) != hipSuccess) return;
            g_prof_made++;
        }
        slot = g_prof_used++;
        (void)hipEventRecord(g_prof_ev[2 * slot], s);
    }
    ~ProfScope() {
        if (slot < 0) return;
        std::lock_guard<std::mutex> lock(g_prof_mu);
        (void)hipEventRecord(g_prof_ev[2 * slot + 1], s);
    }
};

static int threads_for(int fill, int w);
static int grid_for(size_t items, int threads) {
    size_t b = (items + threads - 1) / threads;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// eye geometry / parameters for one call (reference :1533-1541, :1060-1065)
static void eye_setup(EyeArgs& E, double div_percent_signed, double sep_percent_signed, int w) {
    double div_px = (div_percent_signed / 100.0) * (double)w;
    double sep_px = (sep_percent_signed / 100.0) * (double)w;
    E.div32 = (float)div_px;
    E.sep32 = (float)sep_px;
    E.div64 = div_px;
    E.sep64 = sep_px;
    E.asc = div_px < 0 ? 1 : 0;
    E.naive_lim = abs((int)div_px) + 2;
    E.csg_cap = 5 * (int)fabs(div_px) + 25;
    E.enabled = 1;
    E.xoff = E.yoff = 0;
}

// halo of the tiled polylines path: every source column within S of an output pixel can reach it.
// |nd| <= max(|c|, |1-c|) because the normalised depth lies in [0, 1] (flat depth: nd = -c).
static int poly_halo(double div_percent_a, double div_percent_b, double sep_percent, double exponent, double conv, int w) {
    if (!(exponent >= 0.0)) return 1 << 20;  // |nd|^e is unbounded near 0 for e < 0: no finite halo
    double m = fmax(fabs(conv), fabs(1.0 - conv));
    double d = fmax(fabs(div_percent_a), fabs(div_percent_b)) / 100.0 * w;
    double s = d * pow(m, exponent) * 1.0001 + fabs(sep_percent / 100.0 * w);
    if (!(s < 1e6)) return 1 << 20;
    return (int)ceil(s) + 2;
}

static int params_halo(const cs_params* p, int w) {   // ... of a cs_generate call on frames of `w` columns
    return poly_halo(p->divergence * (1 + p->stereo_balance), p->divergence * (1 - p->stereo_balance), p->separation,
                     p->stereo_offset_exponent, p->convergence_point, w);
}
// the per-frame statistics words every workspace starts with
static size_t stats_bytes(size_t n) { return al256(n * ST_WORDS * 4); }
// The stats pre-pass: the words of `frames` frames initialised and, with a depth map of `per_frame` values a frame, its min / max in
// ST_L_MIN / ST_L_MAX (depth == nullptr: the caller's own kernels fill the words).  The reference's latent shifts normalise with
// the min / max of the whole tensor: one frame of b * h * w values.
enum class NanInDepth { DROPPED, POISONS };   // POISONS: a NaN makes the max word a NaN (the latent shifts, torch's min / max)
static void stats_prepass(uint32_t* stats, int frames, const float* depth, size_t per_frame, hipStream_t stream,
                          NanInDepth nan = NanInDepth::DROPPED) {
    hipLaunchKernelGGL(k_stats_init, dim3((frames * ST_WORDS + 255) / 256), dim3(256), 0, stream, stats, frames);
    if (!depth) return;
    const dim3 grid(grid_for(per_frame, 256), frames);
    if (nan == NanInDepth::POISONS)   // the latent shifts, cs_grid_warp, cs_inpaint_prepare: torch's min / max return a NaN
        hipLaunchKernelGGL(k_minmax<true>, grid, dim3(256), 0, stream, depth, (int)per_frame, stats, ST_L_MIN, ST_L_MAX);
    else
        hipLaunchKernelGGL(k_minmax<false>, grid, dim3(256), 0, stream, depth, (int)per_frame, stats, ST_L_MIN, ST_L_MAX);
}
// techniques with a D64 (numba typing) instantiation: the forward-map family, the z-buffered inverse map and -- through the
// general row kernel only, the sweep of full D64 as a literal one-lane replay -- the polylines techniques
// (round 5: also the three techniques no UI string reaches -- none_post / inverse_post: their mapping functions are @njit, the
// float64 offset chain is all numba changes; hybrid_edge_plus = hybrid_edge + polylines_soft, both of which have the dialect)
static bool dialect_d64_ok(int fill) { return fill >= 0 && fill <= CS_FILL_HYBRID_EDGE_PLUS && fill != CS_FILL_GPU_WARP; }
static const char* const DIALECT_MSG = "dialect D64 (flags bits 3/4) exists for the CPU techniques, not for gpu_warp (torch arithmetic in both installs)";
// the flagged-row block of a call of `rows` rows (cs_kernels.h RowBlock: the one description of its layout)
static size_t rowflag_bytes(size_t rows) { return row_block(nullptr, rows).bytes; }

// polylines: tiled fast path + general row kernel over the rows it flagged; everything else: row kernel
// anaglyph scratch of the tiled polylines path: both eyes as uint8 codes side by side
static size_t poly_anaglyph_bytes(int n, int h, int w) { return al256((size_t)n * h * 2 * w * 3); }

// Anaglyph modes of the forward fills and the two `_post` techniques beyond the width their row kernel takes WITH its anaglyph stash (two
// more bytes of LDS per column): the row kernel runs in its side-by-side form into uint8 scratch -- every row, no tile kernel -- and
// k_anaglyph_compose makes the composite, as the polylines techniques do since round 5.  Row-kernel speed, for frames that were refused
// before (round 6: naive_interpolating 7 365 -> 8 104 columns, i.e. an 8K anaglyph; none 10 128 -> 11 578, naive / inverse 8 104 -> 9 004).
static bool ana_wide_fill(int fill) {
    return fill == CS_FILL_NONE || fill == CS_FILL_NAIVE || fill == CS_FILL_NAIVE_INTERPOLATING || fill == CS_FILL_INVERSE ||
           fill == CS_FILL_NONE_POST || fill == CS_FILL_INVERSE_POST;
}
// widest row the LDS-resident row kernel takes, in its anaglyph form (two more bytes of LDS per column) or its side-by-side form
static int row_form_max_width(int fill, int anaglyph) {
    int lo = 0, hi = 1 << 16;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (rowwarp_lds_bytes(fill, mid, anaglyph) <= CS_LDS_BYTES && poly_npt(mid, 1) < 65535) lo = mid; else hi = mid - 1;
    }
    return lo;
}
static bool ana_wide_call(int fill, int anaglyph, int w) { return anaglyph && ana_wide_fill(fill) && w > row_form_max_width(fill, 1); }

// The ONE predicate of the polylines path choice: the tile kernels take a call of dialect `d64` (flags bits 3/4), `w` columns and
// `halo` -- D32 up to k_polytile's halo; the float64 disparity chain (d64 & 1) and numba's typing of the sweep (d64 & 2, round 6:
// k_polypoint<..., SW>, the point kernel's default geometry only) through the point kernel alone.  run_rows, width_refusal and
// generate_chunk's lazy-tile choice all ask it.
static bool polypoint_takes(int halo) { return halo <= polypoint_max_halo() && dev_switch(CS_DEBUG_PT_VARIANT) != PTV_FIRST_GEN; }
static bool poly_tile_takes(int d64, int w, int halo) {
    if (halo > polytile_max_halo() || dev_switch(CS_DEBUG_NO_TILE)) return false;
    if (d64 == 0) return true;
    return polypoint_takes(halo) && (d64 == 1 || polypoint_sweep64_ok(w, halo));
}

static int run_rows(int fill, RowArgs& A, int halo, uint8_t* rowflag, hipStream_t stream, uint8_t* ana_sbs = nullptr,
                    void* replay_scratch = nullptr, size_t replay_surplus = 0) {
    const bool poly = is_poly(fill);
    const size_t rows = (size_t)A.n * A.h;
    const RowBlock B = row_block(rowflag, rows);
    // anaglyph modes of the tiled polylines path (round 5): BOTH kernels -- the tile kernel and the row kernel over the rows it
    // flags -- write the two eyes as uint8 codes side by side into scratch (no mask), and k_anaglyph_compose makes the composite
    // of every row afterwards.  The row kernel then runs in its side-by-side form: no anaglyph stash in LDS (the width limit of
    // the side-by-side modes: polylines_sharp 7 990 instead of 6 395 columns), and its order-dependent stretches go to the replay
    // kernel like those of the other modes.  (Rounds 2-4 let the row kernel write flagged rows in final anaglyph form.)
    // soft / sharp: the point-owner kernel (cs_polypoint.hip) unless the halo is too wide for it or the development switch
    // PTV_FIRST_GEN asks for the first generation (cs_polytile.hip)
    const bool tiled = poly && rowflag && poly_tile_takes(A.d64, A.w, halo);
    const bool ana_tiled = tiled && A.anaglyph && ana_sbs && A.image_f32 && !A.out_u8;
    const bool ana_wide = ana_wide_call(fill, A.anaglyph, A.w) && ana_sbs && A.image_f32 && !A.out_u8;
    const RowArgs Afinal = A;
    if (ana_tiled || ana_wide) {
        A.anaglyph = 0; A.single = -1;
        A.stereo = reinterpret_cast<float*>(ana_sbs); A.stereo_is_u8 = 1; A.no_mask = 1; A.mask = nullptr;
        A.out_h = A.h; A.out_w = 2 * A.w;
        A.eye[0].xoff = 0; A.eye[0].yoff = 0; A.eye[1].xoff = A.w; A.eye[1].yoff = 0;
    }
    // polylines, eyes in separate output slots: the stretches of order-dependent rows are replayed by a kernel of their own
    // (cs_rowwarp.hip k_poly_replay) instead of inside the row kernel
    const bool replay = poly && !A.d64 && replay_scratch && rowflag && !A.anaglyph && !dev_switch(CS_DEBUG_NO_REPLAY_KERNEL) &&
                        poly_replay_bytes(A.n, A.h, A.w, fill == CS_FILL_POLYLINES_SHARP) > 0;
    int hint_T = 0;         // tile width of k_polypoint when it took the call (its hint words are then valid)
    bool cleared = false;   // the flagged-row block (everything in front of its list) has been zeroed
    if (replay) poly_replay_attach(A, fill == CS_FILL_POLYLINES_SHARP, replay_scratch, B, replay_surplus);
    if (tiled && !A.anaglyph) {   // (anaglyph calls arrive here in their side-by-side form)
        hipError_t e = hipMemsetAsync(rowflag, 0, B.clear_bytes, stream);
        if (e != hipSuccess) return fail_hip(e, "rowflag memset");
        cleared = true;
        const RowArgs& T = A;
        if (polypoint_takes(halo))
            e = launch_polypoint(T, halo, B.flags, stream, fill == CS_FILL_POLYLINES_SHARP, B.hints, &hint_T);
        else
            e = launch_polytile(fill == CS_FILL_POLYLINES_SHARP, T, halo, B.flags, stream);
        if (e != hipSuccess) return fail_hip(e, "tiled polylines launch");
        // single-eye modes (left-only / only-right): the tile kernels visit one eye, both depth maps are outputs all the same
        if (A.neyes == 2 && A.single >= 0 && !A.out_u8) {
            const int other = 1 - A.single;
            float* dd = other == 0 ? A.depth_l : A.depth_r;
            if (dd) {
                e = launch_depth_codes(A.eye[other].depth, A.n, A.h, A.w, A.stats, A.scale_from_stats, dd, stream);
                if (e != hipSuccess) return fail_hip(e, "depth-map output launch");
            }
        }
        e = launch_collect_rows(B.flags, (int)rows, B.first, B.list, stream);
        if (e != hipSuccess) return fail_hip(e, "flagged-row collection");
        A.row_list = B.list; A.row_count = B.first;
        const uint32_t* hints = B.hints;
        // (round 6) second tier: the flagged rows through the point kernel once more (k_polypoint_listed) with PP_DCAP2 = 192 instead
        // of 160 slots for pixels under reversed segments and longer per-pixel lists (8 points / 12 segments sharp, 6 / 9 soft); what
        // THAT flags -- B.flags2 and B.hints2, counted in B.point2 -- is collected into the same list for the row kernel.  Depth maps with strong silhouettes
        // (tools/synth.scene8) overflowed the first tier's lists in 15 % (soft) / 48 % (sharp) of the rows at the metric's divergence
        // and sent them to the row kernel: 4 200 / 1 060 frames/s against 5 380 / 4 050 on stepped depth.  polylines_sharp only:
        // for soft the lean row kernel on the hinted tiles' columns is the cheaper second stop (0.96 against 1.16 ms per 16 frames,
        // tools/sessions/r06_s11.sh, s12: 4 100 against 3 750 frames/s; PTV_SOFT_POINT_TIER2 forces the tier for soft, PTV_NO_POINT_TIER2: off)
        // (numba's sweep, d64 & 2: both techniques -- what the tier does not finish takes the dialect row kernel whole, there is no lean pass)
        if (hint_T > 0 && (fill == CS_FILL_POLYLINES_SHARP || (A.d64 & 2) || dev_switch(CS_DEBUG_PT_VARIANT) == PTV_SOFT_POINT_TIER2) &&
            dev_switch(CS_DEBUG_PT_VARIANT) != PTV_NO_POINT_TIER2) {
            e = launch_polypoint_tier2(T, halo, B.flags2, stream, fill == CS_FILL_POLYLINES_SHARP, B.hints2, hint_T, B.list, B.first);
            if (e == hipSuccess) {
                e = launch_collect_rows(B.flags2, (int)rows, B.point2, B.list, stream);
                if (e != hipSuccess) return fail_hip(e, "flagged-row collection (second tier)");
                A.row_count = B.point2;
                hints = B.hints2;
            } else if (e != hipErrorNotSupported) return fail_hip(e, "tiled polylines launch (second tier)");
        }
        // (the lean first pass works on the flagged tiles' column ranges; PTV_LEAN_WHOLE_ROWS: whole rows as in round 4)
        if (hint_T > 0 && dev_switch(CS_DEBUG_PT_VARIANT) != PTV_LEAN_WHOLE_ROWS) {
            A.hint = hints; A.hint_T = hint_T; A.hint_S = halo;
        }
    }
    if ((fill == CS_FILL_NONE || fill == CS_FILL_INVERSE || fill == CS_FILL_NAIVE || fill == CS_FILL_NAIVE_INTERPOLATING) &&
        !dev_switch(CS_DEBUG_NO_TILE) && !ana_wide) {
        // the halo-tile kernel where it applies; 'naive' hands the rows it cannot decide to the row kernel
        const bool flagging = (fill == CS_FILL_NAIVE || fill == CS_FILL_NAIVE_INTERPOLATING) && rowflag;
        if (flagging) {
            hipError_t e = hipMemsetAsync(rowflag, 0, B.clear_bytes, stream);
            if (e != hipSuccess) return fail_hip(e, "rowflag memset");
        }
        hipError_t e = launch_fwdtile(fill, A, halo, flagging ? B.flags : nullptr, stream);
        if (e == hipSuccess) {
            if (!flagging) return CS_OK;
            e = launch_collect_rows(B.flags, (int)rows, B.first, B.list, stream);
            if (e != hipSuccess) return fail_hip(e, "flagged-row collection");
            A.row_list = B.list; A.row_count = B.first;
            // naive_interpolating, second tier (round 5): the flagged rows through the tile kernel once more with a window that holds every
            // hole; what THAT flags (B.naive_flags2(), the retry-flag bytes of the block) is collected into the same list for the row kernel.  On depth
            // saturated to 0 / 1 the holes between a near and a far plateau outgrow the first window in most rows (1 830 frames/s at 4K)
            if (fill == CS_FILL_NAIVE_INTERPOLATING && dev_switch(CS_DEBUG_PT_VARIANT) != PTV_NAIVE_NO_TIER2) {
                e = launch_fwdtile(fill, A, halo, B.naive_flags2(), stream, B.list, B.first);
                if (e == hipSuccess) {
                    e = launch_collect_rows(B.naive_flags2(), (int)rows, B.retry, B.list, stream);
                    if (e != hipSuccess) return fail_hip(e, "flagged-row collection (second tier)");
                    A.row_count = B.retry;
                } else if (e != hipErrorNotSupported) return fail_hip(e, "forward tile kernel launch (second tier)");
            }
        } else if (e != hipErrorNotSupported) return fail_hip(e, "forward tile kernel launch");
    }
    if (A.tilemap) {
        // lazy depth-blur tiles: the row kernels read complete rows of the blurred maps -- fill in the unwritten tiles of the
        // rows they are about to visit (the rows a tile kernel flagged; every row when no tile kernel took the call)
        hipError_t e = launch_lazy_rows(A.row_list, A.row_count, A.n * A.h, A.lazy_gray, const_cast<float*>(A.eye[0].depth),
                                        const_cast<float*>(A.eye[1].depth), A.tilemap, A.stats, A.h, A.w, stream);
        if (e != hipSuccess) return fail_hip(e, "lazy depth rows");
    }
    if (replay && !cleared) {   // (no tile kernel took the call: the block has not been cleared yet)
        hipError_t e0 = hipMemsetAsync(rowflag, 0, B.clear_bytes, stream);
        if (e0 != hipSuccess) return fail_hip(e0, "rowflag memset");
    }
    // (polylines with the replay kernel attached: the lean instantiation first -- evaluation, stretch list, export; the rows it
    // cannot export come back through the retry flags below)
    hipError_t e = launch_rowwarp(fill, A, threads_for(fill, A.w), stream, 0, replay);
    if (e != hipSuccess) return fail_hip(e, "row kernel launch");
    if (replay) {
        e = launch_poly_replay(fill == CS_FILL_POLYLINES_SHARP, A, B, halo, stream);
        if (e != hipSuccess) return fail_hip(e, "stretch replay launch");
        // rows with a stretch the replay kernel gave up on (usually none): once more through the row kernel, export off
        e = launch_collect_rows(B.retry_flags, (int)rows, B.retry, B.list, stream);
        if (e != hipSuccess) return fail_hip(e, "replay retry collection");
        RowArgs R = A;
        R.rp_dump = nullptr; R.row_list = B.list; R.row_count = B.retry; R.hint = nullptr;
        // (one workgroup per CU: on saturated depth a few hundred rows per frame come back -- stretches whose list outgrows the
        // wave form's 64 entries --, 32 workgroups made them the tail of the call; an empty launch of 256 costs 0.03 ms)
        e = launch_rowwarp(fill, R, threads_for(fill, A.w), stream, 256);
        if (e != hipSuccess) return fail_hip(e, "row kernel launch (replay retry)");
    }
    if (ana_tiled || ana_wide) {   // R from one eye, G and B from the other, k / 255, the mask of the composite -- every row
        e = launch_anaglyph_compose(ana_sbs, nullptr, Afinal.n, Afinal.h, Afinal.w, Afinal.anaglyph, Afinal.stereo, Afinal.stereo_is_u8,
                                    Afinal.mask, stream);
        if (e != hipSuccess) return fail_hip(e, "anaglyph composition launch");
    }
    return CS_OK;
}

static int threads_for(int fill, int w) {
    if (w <= 256) return 256;
    if (w <= 1024) return 512;
    // wide rows: the row kernels need 110-128 VGPRs, i.e. 16 waves per CU either way -- as two 512-thread workgroups they
    // overlap each other's barrier phases (measured at 4K: none +7 %, inverse +9 %, naive_interpolating +43 %); naive and
    // the polylines row kernel prefer the single 1024-thread workgroup (naive: -22 % at 512)
    if (fill == CS_FILL_NONE || fill == CS_FILL_INVERSE || fill == CS_FILL_NAIVE_INTERPOLATING || fill == CS_FILL_NONE_POST ||
        fill == CS_FILL_INVERSE_POST)
        return 512;
    return 1024;
}

}  // namespace cs

using namespace cs;

extern "C" {

int cs_version(void) { return CS_ABI_VERSION; }
const char* cs_last_error(void) { return g_err; }

// widest frame the LDS-resident row kernels take; anaglyph modes keep two channels of the first eye per pixel as well
static int max_width_for(int fill, int anaglyph) {
    // (polylines, round 5: the anaglyph modes run both kernels in their side-by-side form and compose afterwards, run_rows above:
    // no anaglyph stash in LDS, the limit of the side-by-side modes.  A call whose halo is too wide for the tile kernels still takes
    // the row kernel's anaglyph form: cs_generate checks that case against `row_form_max_width`)
    if (is_poly(fill)) anaglyph = 0;
    if (ana_wide_fill(fill)) anaglyph = 0;   // (round 6: beyond the stash form's width the row kernel runs side by side + composition, run_rows)
    if (fill == CS_FILL_GPU_WARP) return gpuwarp_max_width();   // (the mesh-quality variant, cs_params.flags bit 2: cs_forward_warp_mesh's limit)
    if (fill == CS_FILL_HYBRID_EDGE) return hybrid_max_width();
    if (fill < 0 || fill > CS_FILL_HYBRID_EDGE_PLUS) return 0;
    return row_form_max_width(fill, anaglyph);
}
// polylines under the float64 disparity chain keep 8 more bytes per column in LDS (cs_rowwarp.hip Poly::xd)
static bool dialect_width_ok(int fill, int w, int anaglyph, int d64) {
    if (!(d64 & 1) || !(is_poly(fill) || is_hybrid(fill))) return true;
    return rowwarp_lds_bytes(fill, w, fill == CS_FILL_HYBRID_EDGE ? 0 : anaglyph) + 8 * (size_t)w + 16 <= CS_LDS_BYTES;
}
// The ONE width predicate of cs_generate: nullptr when a frame of `w` columns with p's technique, mode, dialect flags
// and disparity parameters is accepted, else the reason.  cs_max_width_params searches it, so a caller that pre-validates gets
// exactly the answer the call itself would give.
static const char* width_refusal(const cs_params* p, int w) {
    const bool ana = is_anaglyph(p->mode);
    if (w > max_width_for(p->fill, ana) || !dialect_width_ok(p->fill, w, ana, (p->flags >> 3) & 3))
        return "frame too wide for the LDS-resident row kernel";
    if (is_poly(p->fill) && ana && w > row_form_max_width(p->fill, 1)) {
        // an anaglyph wider than the row kernel's anaglyph form: only through the tile kernels (run_rows' tiled anaglyph path;
        // cs_generate's images are float32)
        if (!poly_tile_takes((p->flags >> 3) & 3, w, params_halo(p, w)))
            return "frame too wide for the LDS-resident row kernel (anaglyph form)";
    }
    return nullptr;
}
int cs_max_width_params(const cs_params* p) {
    if (!p || p->fill < 0 || p->fill > CS_FILL_HYBRID_EDGE_PLUS) return 0;
    int lo = 0, hi = 1 << 16;   // (monotone: LDS bytes and the halo both grow with the width)
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (!width_refusal(p, mid)) lo = mid; else hi = mid - 1;
    }
    return lo;
}
int cs_max_width(int fill) { return max_width_for(fill, 1); }
int cs_max_width_mode(int fill, int mode) { return max_width_for(fill, is_anaglyph(mode)); }

int cs_output_shape(const cs_params* p, int* out_h, int* out_w, int* mask_h, int* mask_w) {
    if (!p) return fail(CS_EINVAL, "null params");
    int oh = p->h, ow = p->w;
    switch (p->mode) {
    case CS_MODE_LEFT_RIGHT: case CS_MODE_RIGHT_LEFT: ow = 2 * p->w; break;
    case CS_MODE_TOP_BOTTOM: case CS_MODE_BOTTOM_TOP: oh = 2 * p->h; break;
    case CS_MODE_RED_CYAN_ANAGLYPH: case CS_MODE_CYAN_RED_REVERSEANAGLYPH:
    case CS_MODE_LEFT_ONLY: case CS_MODE_ONLY_RIGHT: break;
    default: return fail(CS_EINVAL, "Unknown mode");
    }
    if (out_h) *out_h = oh;
    if (out_w) *out_w = ow;
    // CPU techniques: the mask is computed from the assembled output (GenerateStereo.py:355-361);
    // gpu_warp: left_mask | right_mask, eye-shaped (stereoimage_generation.py:1090).
    if (mask_h) *mask_h = p->fill == CS_FILL_GPU_WARP ? p->h : oh;
    if (mask_w) *mask_w = p->fill == CS_FILL_GPU_WARP ? p->w : ow;
    return CS_OK;
}


// hyb / gpuwarp / ana_sbs / replay: the technique's scratch behind the depth maps (absent ones are empty) -- the splat result of
// hybrid_edge, gpu_warp's scratch, both eyes as uint8 codes side by side (has_ana_sbs: run_rows composes this call's anaglyph from
// them) and the stretch-replay scratch of the polylines techniques: the last item, so that a larger workspace extends its pool
struct WsLayout {
    size_t rowflag, gray_src, gray, L, R, wl, wr, tilemap, hyb, gpuwarp, ana_sbs, replay, total;
    bool has_ana_sbs;
};
// Scratch of one chunk of frames (everything but the per-frame statistics words, which stay one array for the whole call
// at the start of the workspace so that callers find them at a fixed place).
static WsLayout ws_layout(const cs_params* p) {
    WsLayout W;
    size_t hw = (size_t)p->h * p->w, n = p->n, o = 0;
    W.rowflag = o; o += rowflag_bytes(n * (size_t)p->h);
    bool resize = p->depth_h != p->h || p->depth_w != p->w;
    W.gray_src = o; if (resize) o += al256(n * (size_t)p->depth_h * p->depth_w * 4);
    const bool blur = blur_on(p);
    // (the gray buffer sits BETWEEN the blurred maps: the lazy-tile readers address either of a pair with a 32-bit offset)
    W.L = o; if (blur) o += al256(n * hw * 4);
    W.gray = o; o += al256(n * hw * 4);
    W.R = o; if (blur) o += al256(n * hw * 4);
    W.wl = o; if (blur) o += al256(n * hw * 4);
    W.wr = o; if (blur) o += al256(n * hw * 4);
    W.tilemap = o; if (blur) o += al256(blur_tilemap_bytes(p->n, p->h, p->w));
    const bool poly = is_poly(p->fill), ana = is_anaglyph(p->mode);
    W.hyb = o; if (is_hybrid(p->fill)) o += al256(hybrid_workspace_bytes(p->n, p->h, p->w));
    W.gpuwarp = o; if (p->fill == CS_FILL_GPU_WARP) o += al256(gpuwarp_workspace_bytes(p->n, p->h, p->w, p->batch_size, p->flags & 4));
    // (the anaglyphs of the polylines techniques, and those of the forward fills too wide for the row kernel's stash form)
    W.has_ana_sbs = (poly && ana) || ana_wide_call(p->fill, ana, p->w);
    W.ana_sbs = o; if (W.has_ana_sbs) o += poly_anaglyph_bytes(p->n, p->h, p->w);
    W.replay = o; if (poly) o += al256(poly_replay_bytes(p->n, p->h, p->w, p->fill == CS_FILL_POLYLINES_SHARP));
    W.total = o;
    return W;
}

// ---- frame chunks: the pre-pass of chunk c + 1 under the warp of chunk c ---------------------------------------------
// A call can cut its batch into chunks of frames -- every quantity of the path is per frame (gpu_warp: per reference
// sub-batch, so its chunks are multiples of batch_size) -- and issue the pre-pass of every chunk (gray depth, edge bit rows,
// tile classification, fused blur: HBM-bound) on an auxiliary stream, the warps on the caller's stream, one event per chunk
// in between, so that the pre-pass of chunk c + 1 runs under the warp of chunk c.  Fork / join is by events only (legal
// under stream capture); all work the call enqueues is ordered before whatever the caller enqueues next on its stream.
// MEASURED (round 3, profiles/r03_overlap.txt): the schedule is correct and overlaps, and it is a zero-sum game -- the warp
// kernels are bound by the latency of their resident workgroups (k_polypoint: time x workgroups per CU is constant from 3
// to 6 workgroups per CU), every co-resident pre-pass workgroup takes wave slots and memory queue from them: 64 4K frames
// polylines_soft 14.3 ms in one chunk, 14.5 / 14.8 / 15.1 / 15.6 ms in 2 / 4 / 8 / 16 chunks with the auxiliary stream at
// the highest priority, 14.3 / 14.5 / 14.8 in 2 / 4 / 8 at the caller's priority; cfg 3 / 4 / 5 gain 0.1 - 2 %.  The
// default is therefore ONE chunk on the caller's stream; cs_debug_set(CS_DEBUG_CHUNKS, k) with k > 1 cuts k chunks
// (+100: auxiliary stream at the default priority instead of the highest).
struct ChunkPlan { int nch, cf; };
static ChunkPlan plan_chunks(const cs_params* p) {
    const int n = p->n, forced = dev_switch(CS_DEBUG_CHUNKS) % 100;   // (+100: auxiliary stream at the default priority)
    int unit = 1;
    if (p->fill == CS_FILL_GPU_WARP) unit = warp_group(p);
    if (forced <= 1 || n < 2 * unit) return ChunkPlan{1, n};
    int cf = (n + forced - 1) / forced;
    cf = (cf + unit - 1) / unit * unit;
    const int nch = (n + cf - 1) / cf;
    if (nch < 2) return ChunkPlan{1, n};
    return ChunkPlan{nch, cf};
}
static size_t ws_total(const cs_params* p) {
    const ChunkPlan C = plan_chunks(p);
    cs_params q = *p;
    q.n = C.cf;
    return stats_bytes(p->n) + (size_t)C.nch * ws_layout(&q).total;
}

// the auxiliary stream (highest priority the device offers) and its fork / ready events: one set per device, created on
// first use, shared by every caller (the events order each call's own work; sharing the stream only serialises the
// pre-passes of concurrent callers)
static const int AUX_MAX_DEV = 16, AUX_EVENTS = 8;
struct AuxStream { hipStream_t s; hipEvent_t fork, ready[AUX_EVENTS]; bool ok; };
static std::mutex g_aux_mu;
static AuxStream g_aux[AUX_MAX_DEV][2];
// low = 0: the highest priority the device offers, 1: the lowest (the pre-pass only fills what the warp leaves free)
static AuxStream* aux_stream(int low) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= AUX_MAX_DEV) return nullptr;
    std::lock_guard<std::mutex> lock(g_aux_mu);
    AuxStream& A = g_aux[dev][low ? 1 : 0];
    if (A.ok) return &A;
    int least = 0, greatest = 0;   // (the numerically lowest value is the highest priority)
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; }
    if (hipStreamCreateWithPriority(&A.s, hipStreamNonBlocking, low ? least : greatest) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&A.fork, hipEventDisableTiming) != hipSuccess) return nullptr;
    for (int i = 0; i < AUX_EVENTS; i++)
        if (hipEventCreateWithFlags(&A.ready[i], hipEventDisableTiming) != hipSuccess) return nullptr;
    A.ok = true;
    return &A;
}

size_t cs_workspace_bytes(const cs_params* p) { return (p && p->n > 0) ? ws_total(p) : 0; }

// Lazy tiles: the tile kernels (cs_polypoint / cs_polytile / cs_fwdtile) read the edge-free tiles of the blurred depth -- a scaled
// copy of the gray depth -- from the gray depth itself, so the blur leaves them unwritten and hands over the map of the tiles it
// did write; run_rows completes the rows that still go to a row kernel.  (Round 2 measured the selector in k_gpuwarp and in the
// hybrid splat as dearer than the copy; with both kernels restructured at the end of round 3 -- loads first, four workgroups per
// CU -- it is cheaper.)  This call's warp reads the map:
static bool lazy_tiles_wanted(const cs_params* p, int halo) {
    const int fill = p->fill, w = p->w, d64 = (p->flags >> 3) & 3;
    const bool tile_fill = is_poly(fill) || fill == CS_FILL_NONE || fill == CS_FILL_INVERSE || fill == CS_FILL_NAIVE || fill == CS_FILL_NAIVE_INTERPOLATING;
    // gpu_warp (scatter-round warp, rows of at most 4096 columns) reads the map too since the end of round 3: the kernel is
    // bound by its dependent chains, not by its instruction count -- the selector costs less than the copy of the tiles
    const bool warp_lazy = fill == CS_FILL_GPU_WARP && !(p->flags & 4) && w <= gpuwarp_lazy_max_width() && !dev_switch(CS_DEBUG_GPUWARP_FULL_MAPS);
    // hybrid_edge through the fused splat tile kernel (two-eye layouts): the same; the disabled-eye path and the unfused
    // forms read complete maps, so the map is only used when both eyes run
    const bool two_eyes = !(p->divergence * (1 + p->stereo_balance) < 0.001) && !(p->divergence * (1 - p->stereo_balance) < 0.001);
    const bool hyb_lazy = fill == CS_FILL_HYBRID_EDGE && two_eyes && !dev_switch(CS_DEBUG_HYBRID_FULL_MAPS) &&
                          hybrid_fused_ok(p->n, w, halo, is_anaglyph(p->mode), -1, d64, 0);
    // (round 6: the polylines techniques under a dialect flag too -- the point kernel's dialect instantiations share the tile function,
    // lazy loads included, and run_rows completes the rows of any call a row kernel ends up taking; the other techniques' dialect
    // kernels keep complete maps: 0.94 of 17.1 ms per 64 frames under D64, profiles/r06_s39/)
    const bool dialect_lazy = d64 == 0 || (is_poly(fill) && poly_tile_takes(d64, w, halo));
    // (single-eye modes read complete maps; the readers address either blurred map from the gray depth between them with a
    // 32-bit offset: ws_layout)
    return (tile_fill || warp_lazy || hyb_lazy) && dialect_lazy && !dev_switch(CS_DEBUG_NO_TILE) && !dev_switch(CS_DEBUG_BLUR_FULL_COPY) &&
           p->mode != CS_MODE_LEFT_ONLY && p->mode != CS_MODE_ONLY_RIGHT && al256((size_t)p->n * p->h * w * 4) < (1ull << 32) - (1u << 20);
}

// One chunk of frames: the pre-pass on `sp`, the warp on `stream` (the same stream, or `ready` recorded on sp and awaited
// by stream in between).  `stats`: the chunk's slice of the call's statistics words; `ws`: the chunk's scratch (ws_layout).
static int generate_chunk(const cs_params* p, const float* image, const float* depth, float* stereo, float* depth_l,
                          float* depth_r, float* mask, uint32_t* stats, char* ws, int out_h, int out_w, hipStream_t sp,
                          hipStream_t stream, hipEvent_t ready, size_t surplus = 0) {
    int rc;
    const WsLayout W = ws_layout(p);
    float* gray = (float*)(ws + W.gray);
    uint32_t* const tilemap = (uint32_t*)(ws + W.tilemap);
    const int n = p->n, h = p->h, w = p->w, hw = h * w;
    const bool gpu_warp = p->fill == CS_FILL_GPU_WARP, blur = blur_on(p);
    const bool resize = p->depth_h != h || p->depth_w != w;
    const int halo = params_halo(p, w);
    // the blur's plan, made once.  The reference's callers pass the strength as the mask width too (:1051, :1479).  An RGB depth
    // map at the frames' size: the gray conversion can build the blur's edge bit rows as well (one pass over the depth input)
    const BlurParams prm = {p->depth_blur_strength, p->depth_blur_edge_threshold, p->depth_blur_strength, p->depth_blur_falloff,
                            p->depth_blur_vert_smooth};
    const bool blur_map = !dev_switch(CS_DEBUG_BLUR_FULL_COPY);
    const BlurPlan B = blur ? blur_plan(prm, n, h, w, (float*)(ws + W.wl), (float*)(ws + W.wr), blur_map, true, !resize && p->depth_c == 3)
                            : BlurPlan{};
    // gray depth and its statistics
    stats_prepass(stats, n, nullptr, 0, sp);   // (the gray conversion below fills the words)
    if (resize) {
        float* gs = (float*)(ws + W.gray_src);
        int shw = p->depth_h * p->depth_w;
        hipLaunchKernelGGL(k_gray, dim3(grid_for(shw / 32 + 1, 256), n), dim3(256), 0, sp, depth, gs, shw, p->depth_c, stats, 0);
        hipLaunchKernelGGL(k_resize_bilinear, dim3(grid_for(hw, 256), n), dim3(256), 0, sp, gs, p->depth_h, p->depth_w, gray, h, w, stats);
    } else if (B.pre_edges) {
        hipError_t e = launch_gray_edges(B, depth, gray, stats, sp);
        if (e != hipSuccess) return fail_hip(e, "gray + edge pass");
    } else {
        // (>= 8 float4 groups per thread: the per-workgroup min/max reduction is amortised -- 3x faster at 1080p)
        hipLaunchKernelGGL(k_gray, dim3(grid_for(hw / 32 + 1, 256), n), dim3(256), 0, sp, depth, gray, hw, p->depth_c, stats, 1);
    }
    hipLaunchKernelGGL(k_finalize_stats, dim3((n + 63) / 64), dim3(64), 0, sp, stats, n, gpu_warp ? warp_group(p) : 0, blur ? 1 : 0);
    // depth blur
    const float *dL = gray, *dR = gray;
    int scale_from_stats = 1, lazy = 0;
    if (blur) {
        float *L = (float*)(ws + W.L), *R = (float*)(ws + W.R);
        rc = launch_blur(B, gray, L, R, stats, sp, blur_map ? tilemap : nullptr, lazy_tiles_wanted(p, halo) ? &lazy : nullptr);
        if (rc) return fail_blur(rc);
        dL = L; dR = R;
        scale_from_stats = 0;  // the blur kernel already wrote scaled depth
        if (lazy && g_prof_on.load(std::memory_order_relaxed)) {   // (measurement: cs_profile_tiles; outside the timed kernel scope)
            std::lock_guard<std::mutex> lock(g_prof_mu);
            if (g_prof_tiles) {
                const int words = blur_tilemap_words(w), rows = (int)(blur_tilemap_bytes(n, h, w) / ((size_t)words * 4));
                hipLaunchKernelGGL(k_prof_count_tiles, dim3((rows * words + 255) / 256), dim3(256), 0, sp, (const uint32_t*)tilemap,
                                   rows, words, (w + 63) / 64, g_prof_tiles);
                g_prof_tiles_any = true; g_prof_tiles_stream = sp;
            }
        }
    }
    // hand-over
    if (sp != stream) {   // the warp of this chunk waits for its pre-pass; the next chunk's pre-pass runs under it
        hipError_t e = hipEventRecord(ready, sp);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, ready, 0);
        if (e != hipSuccess) return fail_hip(e, "chunk hand-over");
    }
    // warp
    ProfScope prof(stream);
    if (gpu_warp) {
        rc = launch_gpuwarp_node(p, image, dL, dR, scale_from_stats, stats, stereo, depth_l, depth_r, mask, out_h, out_w,
                                 ws + W.gpuwarp, stream, lazy ? tilemap : nullptr, lazy ? gray : nullptr, lazy ? blur_tilemap_words(w) : 0);
        if (rc) return fail(rc, "gpu_warp launch failed");
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? CS_OK : fail_hip(e, "cs_generate");
    }

    RowArgs A;
    memset(&A, 0, sizeof(A));
    A.n = n; A.h = h; A.w = w;
    A.image_f32 = image;
    A.stats = stats; A.stats_rw = stats;
    A.scale_from_stats = scale_from_stats;
    A.e32 = (float)p->stereo_offset_exponent;
    A.conv32 = (float)p->convergence_point;
    A.e64 = p->stereo_offset_exponent;
    A.d64 = (p->flags >> 3) & 3;
    A.neyes = 2;
    const double left_div = p->divergence * (1 + p->stereo_balance), right_div = p->divergence * (1 - p->stereo_balance);
    eye_setup(A.eye[0], +1 * left_div, -1 * p->separation, w);
    eye_setup(A.eye[1], -1 * right_div, p->separation, w);
    A.eye[0].enabled = !(left_div < 0.001);
    A.eye[1].enabled = !(right_div < 0.001);
    A.eye[0].depth = dL; A.eye[0].st_min = ST_L_MIN; A.eye[0].st_max = ST_L_MAX;
    A.eye[1].depth = dR; A.eye[1].st_min = ST_R_MIN; A.eye[1].st_max = ST_R_MAX;
    A.stereo = stereo; A.mask = mask; A.depth_l = depth_l; A.depth_r = depth_r;
    A.stereo_is_u8 = (p->flags & 2) ? 1 : 0;
    A.out_h = out_h; A.out_w = out_w;
    A.single = -1;
    A.dbg = dev_switch(CS_DEBUG_DBG);
    if (lazy) { A.tilemap = tilemap; A.lazy_gray = gray; A.tm_words = blur_tilemap_words(w); }
    switch (p->mode) {
    case CS_MODE_LEFT_RIGHT: A.eye[1].xoff = w; break;
    case CS_MODE_RIGHT_LEFT: A.eye[0].xoff = w; break;
    case CS_MODE_TOP_BOTTOM: A.eye[1].yoff = h; break;
    case CS_MODE_BOTTOM_TOP: A.eye[0].yoff = h; break;
    case CS_MODE_RED_CYAN_ANAGLYPH: A.anaglyph = 1; break;
    case CS_MODE_CYAN_RED_REVERSEANAGLYPH: A.anaglyph = 2; break;
    case CS_MODE_LEFT_ONLY: A.single = 0; break;
    case CS_MODE_ONLY_RIGHT: A.single = 1; break;
    }
    if (is_hybrid(p->fill)) {
        rc = launch_hybrid(A, ws + W.hyb, stream, p->fill == CS_FILL_HYBRID_EDGE_PLUS, halo);
        if (rc) return fail(rc, "hybrid_edge launch failed");
    } else {
        rc = run_rows(p->fill, A, halo, (uint8_t*)(ws + W.rowflag), stream, W.has_ana_sbs ? (uint8_t*)(ws + W.ana_sbs) : nullptr,
                      ws + W.replay, surplus);
        if (rc) return rc;
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_generate");
}

int cs_generate(const cs_params* p, const float* image, const float* depth, float* stereo, float* depth_l,
                float* depth_r, float* mask, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !image || !depth || !stereo || !depth_l || !depth_r || !mask || !workspace) return fail(CS_EINVAL, "null pointer");
    if (p->n <= 0 || p->h <= 0 || p->w <= 0 || p->depth_h <= 0 || p->depth_w <= 0 || p->depth_c <= 0)
        return fail(CS_EINVAL, "non-positive size");
    if (p->fill < 0 || p->fill > CS_FILL_HYBRID_EDGE_PLUS) return fail(CS_EINVAL, "unknown fill technique");
    int out_h, out_w, mask_h, mask_w;
    int rc = cs_output_shape(p, &out_h, &out_w, &mask_h, &mask_w);
    if (rc) return rc;
    if (const char* why = width_refusal(p, p->w)) return fail(CS_ELIMIT, why);
    if (workspace_bytes < ws_total(p)) return fail(CS_EWORKSPACE, "workspace too small");
    if (p->fill == CS_FILL_GPU_WARP && (p->flags & 2)) return fail(CS_EINVAL, "gpu_warp colours are not k/255: no uint8 stereoscope output");
    if ((p->flags & 24) && !dialect_d64_ok(p->fill))
        return fail(CS_EINVAL, DIALECT_MSG);
    char* const ws = (char*)workspace;
    uint32_t* const stats = (uint32_t*)ws;
    char* const scratch = ws + stats_bytes(p->n);
    const ChunkPlan C = plan_chunks(p);
    // (one chunk: whatever the caller's workspace holds beyond cs_workspace_bytes extends the stretch-replay pool -- the last item
    // of the layout -- so that a caller who expects tie-heavy depth maps can give every flagged row room to export)
    if (C.nch == 1) return generate_chunk(p, image, depth, stereo, depth_l, depth_r, mask, stats, scratch, out_h, out_w, stream, stream, nullptr,
                                          workspace_bytes - ws_total(p));

    // mode (CS_DEBUG_CHUNKS / 100): 0 = pre-passes on the highest-priority auxiliary stream, warps on the caller's stream;
    // 1 = pre-passes on an auxiliary stream of the default priority; 2 = pre-passes at the default priority AND the warps on
    // the highest-priority auxiliary stream (the warp keeps its workgroup slots, the pre-pass only fills what is left)
    const int mode = dev_switch(CS_DEBUG_CHUNKS) / 100;
    // The auxiliary streams and their fork / ready events are one set per device: two host threads interleaving their
    // hipEventRecord / hipStreamWaitEvent pairs on them would wait for each other's records.  The chunked schedule (a development
    // switch) therefore enqueues under one lock, from the fork to the join -- host-side enqueueing only, the GPU work itself
    // still overlaps; the shared events also make this path unfit for stream capture (the default single-chunk path is).
    static std::mutex chunk_mu;
    std::lock_guard<std::mutex> chunk_lock(chunk_mu);
    AuxStream* const X = aux_stream(mode >= 1);
    AuxStream* const Wp = mode == 2 ? aux_stream(0) : nullptr;
    if (!X || (mode == 2 && !Wp)) return fail_hip(hipGetLastError(), "auxiliary stream");
    hipStream_t warp_stream = Wp ? Wp->s : stream;
    // fork: the pre-passes start after everything the caller has enqueued so far (inputs, the previous call's use of the
    // workspace); join: the last chunk's warp waits for the last pre-pass, and the auxiliary stream holds nothing else
    hipError_t e = hipEventRecord(X->fork, stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(X->s, X->fork, 0);
    if (e == hipSuccess && Wp) e = hipStreamWaitEvent(Wp->s, X->fork, 0);
    if (e != hipSuccess) return fail_hip(e, "chunk fork");
    cs_params q = *p;
    q.n = C.cf;
    const size_t chunk_ws = ws_layout(&q).total;
    const size_t in_px = (size_t)p->h * p->w, d_px = (size_t)p->depth_h * p->depth_w * p->depth_c;
    const size_t st_px = (size_t)out_h * out_w * 3, mk_px = (size_t)mask_h * mask_w;
    const size_t st_bytes = (p->flags & 2) ? 1 : 4;   // uint8 stereoscope codes (flags bit 1) or float32
    rc = CS_OK;
    for (int c = 0; c < C.nch && rc == CS_OK; c++) {
        const int f0 = c * C.cf;
        q.n = (f0 + C.cf <= p->n) ? C.cf : p->n - f0;
        rc = generate_chunk(&q, image + f0 * in_px * 3, depth + f0 * d_px, (float*)((char*)stereo + f0 * st_px * st_bytes),
                            depth_l + f0 * in_px * 3, depth_r + f0 * in_px * 3, mask + f0 * mk_px, stats + (size_t)f0 * ST_WORDS,
                            scratch + (size_t)c * chunk_ws, out_h, out_w, X->s, warp_stream, X->ready[c % AUX_EVENTS]);
    }
    // join: whatever was enqueued on the auxiliary streams precedes the caller's next work (also after a failure)
    if (Wp) {
        if (hipEventRecord(Wp->fork, Wp->s) == hipSuccess) (void)hipStreamWaitEvent(stream, Wp->fork, 0);
    }
    if (rc != CS_OK || Wp) {
        if (hipEventRecord(X->ready[0], X->s) == hipSuccess) (void)hipStreamWaitEvent(stream, X->ready[0], 0);
    }
    return rc;
}

// [statistics][flagged-row block][technique scratch: the splat result of hybrid_edge / the replay scratch of polylines]
struct AsdLayout { size_t rowflag, tech, total; };   // (the statistics at 0)
static AsdLayout asd_layout(int n, int h, int w, int fill) {
    AsdLayout W;
    W.rowflag = stats_bytes(n);
    W.tech = W.rowflag + rowflag_bytes((size_t)n * h);
    W.total = W.tech;
    if (is_hybrid(fill)) W.total += al256(hybrid_workspace_bytes(n, h, w));
    if (is_poly(fill)) W.total += al256(poly_replay_bytes(n, h, w, fill == CS_FILL_POLYLINES_SHARP));
    return W;
}
size_t cs_asd_workspace_bytes_for(int n, int h, int w, int fill) { return asd_layout(n, h, w, fill).total; }
size_t cs_asd_workspace_bytes(int n, int h, int w) {   // enough for any technique
    const size_t a = cs_asd_workspace_bytes_for(n, h, w, CS_FILL_HYBRID_EDGE), b = cs_asd_workspace_bytes_for(n, h, w, CS_FILL_POLYLINES_SHARP);
    return a > b ? a : b;
}

int cs_apply_stereo_divergence(const uint8_t* image_u8, const float* depth, int n, int h, int w, double divergence,
                               double separation, double exponent, int fill, double convergence, uint8_t* out_u8,
                               void* workspace, size_t workspace_bytes, void* stream_) {
    return cs_apply_stereo_divergence2(image_u8, depth, n, h, w, divergence, separation, exponent, fill, convergence, 0, out_u8,
                                       workspace, workspace_bytes, stream_);
}

int cs_apply_stereo_divergence2(const uint8_t* image_u8, const float* depth, int n, int h, int w, double divergence,
                                double separation, double exponent, int fill, double convergence, int dialect,
                                uint8_t* out_u8, void* workspace, size_t workspace_bytes, void* stream_) {
    if (dialect < 0 || dialect > 3) return fail(CS_EINVAL, "dialect: 0 (D32), 1 (float64 disparities), 2 (int64 sums), 3 (D64)");
    if (dialect && !dialect_d64_ok(fill))
        return fail(CS_EINVAL, DIALECT_MSG);
    hipStream_t stream = (hipStream_t)stream_;
    if (!image_u8 || !depth || !out_u8 || !workspace) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (fill < 0 || fill > CS_FILL_HYBRID_EDGE_PLUS || fill == CS_FILL_GPU_WARP) return fail(CS_EINVAL, "unknown fill technique");
    if (w > max_width_for(fill, 0) || !dialect_width_ok(fill, w, 0, dialect)) return fail(CS_ELIMIT, "frame too wide for the LDS-resident row kernel");
    const AsdLayout W = asd_layout(n, h, w, fill);
    if (workspace_bytes < W.total) return fail(CS_EWORKSPACE, "workspace too small");
    char* const ws = (char*)workspace;
    uint32_t* stats = (uint32_t*)ws;
    stats_prepass(stats, n, depth, (size_t)h * w, stream);
    RowArgs A;
    memset(&A, 0, sizeof(A));
    A.n = n; A.h = h; A.w = w;
    A.image_u8 = image_u8;
    A.stats = stats; A.stats_rw = stats;
    A.scale_from_stats = 0;
    A.e32 = (float)exponent;
    A.conv32 = (float)convergence;
    A.e64 = exponent;
    A.d64 = dialect;
    A.neyes = 1;
    eye_setup(A.eye[0], divergence, separation, w);
    A.eye[0].depth = depth; A.eye[0].st_min = ST_L_MIN; A.eye[0].st_max = ST_L_MAX;
    A.out_u8 = out_u8;
    A.single = -1;
    A.dbg = dev_switch(CS_DEBUG_DBG);
    if (is_hybrid(fill)) {
        int rc = launch_hybrid(A, ws + W.tech, stream, fill == CS_FILL_HYBRID_EDGE_PLUS);
        if (rc) return fail(rc, "hybrid_edge launch failed");
    } else {
        int halo = poly_halo(divergence, divergence, separation, exponent, convergence, w);
        int rc = run_rows(fill, A, halo, (uint8_t*)(ws + W.rowflag), stream, nullptr, is_poly(fill) ? ws + W.tech : nullptr);   // (the others have no replay scratch)
        if (rc) return rc;
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_apply_stereo_divergence");
}

size_t cs_blur_workspace_bytes(int n, int h, int w) { return stats_bytes(n) + 2 * al256((size_t)n * h * w * 4); }

int cs_directional_blur(const float* depth, int n, int h, int w, double blur_strength, double edge_threshold,
                        double blur_mask_width, double falloff_exponent, int vert_smooth_px, float* out_l, float* out_r, void* workspace,
                        size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!depth || !out_l || !out_r || !workspace) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (workspace_bytes < cs_blur_workspace_bytes(n, h, w)) return fail(CS_EWORKSPACE, "workspace too small");
    size_t hw = (size_t)h * w;
    if (blur_strength <= 0) {  // reference :1194 returns the input twice
        hipError_t e1 = hipMemcpyAsync(out_l, depth, n * hw * 4, hipMemcpyDeviceToDevice, stream);
        hipError_t e2 = hipMemcpyAsync(out_r, depth, n * hw * 4, hipMemcpyDeviceToDevice, stream);
        return (e1 == hipSuccess && e2 == hipSuccess) ? CS_OK : fail_hip(e1 != hipSuccess ? e1 : e2, "cs_directional_blur");
    }
    char* ws = (char*)workspace;
    uint32_t* stats = (uint32_t*)ws;
    float* wl = (float*)(ws + stats_bytes(n));
    float* wr = wl + al256(n * hw * 4) / 4;
    stats_prepass(stats, n, nullptr, 0, stream);   // (launch_blur accumulates the outputs' min / max)
    const BlurParams prm = {blur_strength, edge_threshold, blur_mask_width, falloff_exponent, vert_smooth_px};
    int rc = launch_blur(blur_plan(prm, n, h, w, wl, wr, false, false, false), depth, out_l, out_r, stats, stream);
    if (rc) return fail_blur(rc);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_directional_blur");
}

size_t cs_blur_scipy_workspace_bytes(int n, int h, int w) { return scipyblur_workspace_bytes(n, h, w); }

int cs_directional_blur_scipy(const float* depth, int n, int h, int w, double blur_strength, double edge_threshold,
                              double blur_mask_width, double falloff_exponent, int vert_smooth_px, float* out_l, float* out_r,
                              void* workspace, size_t workspace_bytes, void* stream_) {
    if (!depth || !out_l || !out_r || !workspace) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (workspace_bytes < cs_blur_scipy_workspace_bytes(n, h, w)) return fail(CS_EWORKSPACE, "workspace too small");
    if (!(blur_strength > 0.0)) return fail(CS_EINVAL, "blur_strength <= 0: the reference returns the depth map itself (:1374); the caller does the same");
    if (!(blur_strength < 1e6) || !(blur_mask_width < 1e6)) return fail(CS_EINVAL, "blur_strength / blur_mask_width out of range");
    int rc = launch_scipyblur(depth, n, h, w, blur_strength, edge_threshold, blur_mask_width, falloff_exponent, vert_smooth_px,
                              out_l, out_r, workspace, (hipStream_t)stream_);
    if (rc == CS_EINVAL) return fail(rc, "blur_strength rounds to a box of 0 taps: the reference fails there too (scipy: no filter weights given)");
    return rc ? fail(rc, "cs_directional_blur_scipy launch failed") : CS_OK;
}

size_t cs_warp_workspace_bytes(int n, int h, int w) { return stats_bytes(n) + al256(gpuwarp_workspace_bytes(n, h, w, n, 0)); }
size_t cs_warp_mesh_workspace_bytes(int n, int h, int w) { return stats_bytes(n) + al256(gpuwarp_workspace_bytes(n, h, w, n, 1)); }

static int forward_warp_common(const float* image, const float* depth, int n, int h, int w, double divergence_px,
                               double separation_px, double exponent, double convergence, int mesh, double grad_thr,
                               float* warped, uint8_t* gap_mask, void* workspace, size_t workspace_bytes, hipStream_t stream,
                               int max_stretch = 8) {
    if (!image || !depth || !warped || !gap_mask || !workspace) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (mesh && (h < 2 || w < 2)) return fail(CS_EINVAL, "the mesh warp needs at least 2 x 2 pixels");
    if (mesh && !(grad_thr >= 0.0)) return fail(CS_EINVAL, "gradient_threshold must be >= 0");
    if (w > (mesh ? meshwarp_max_width() : gpuwarp_max_width())) return fail(CS_ELIMIT, "frame too wide for the LDS-resident row kernel");
    if (workspace_bytes < (mesh ? cs_warp_mesh_workspace_bytes(n, h, w) : cs_warp_workspace_bytes(n, h, w)))
        return fail(CS_EWORKSPACE, "workspace too small");
    uint32_t* stats = (uint32_t*)workspace;
    stats_prepass(stats, n, depth, (size_t)h * w, stream);
    int rc = launch_gpuwarp_plain(image, depth, n, h, w, divergence_px, separation_px, exponent, convergence, warped,
                                  gap_mask, stats, (char*)workspace + stats_bytes(n), stream, mesh, grad_thr, max_stretch);
    if (rc == CS_ELIMIT) return fail(rc, "gpu_warp: gradient_threshold above 13 with max_stretch above 16 is not supported (more than 16 effective scatter rounds)");
    if (rc) return fail(rc, "gpu_warp launch failed");
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_forward_warp");
}

int cs_forward_warp(const float* image, const float* depth, int n, int h, int w, double divergence_px,
                    double separation_px, double exponent, double convergence, float* warped, uint8_t* gap_mask,
                    void* workspace, size_t workspace_bytes, void* stream_) {
    return forward_warp_common(image, depth, n, h, w, divergence_px, separation_px, exponent, convergence, 0, 1.5, warped,
                               gap_mask, workspace, workspace_bytes, (hipStream_t)stream_);
}

int cs_forward_warp2(const float* image, const float* depth, int n, int h, int w, double divergence_px,
                     double separation_px, double exponent, double convergence, double gradient_threshold, int max_stretch,
                     float* warped, uint8_t* gap_mask, void* workspace, size_t workspace_bytes, void* stream_) {
    return forward_warp_common(image, depth, n, h, w, divergence_px, separation_px, exponent, convergence, 0, gradient_threshold,
                               warped, gap_mask, workspace, workspace_bytes, (hipStream_t)stream_, max_stretch);
}

int cs_forward_warp_mesh(const float* image, const float* depth, int n, int h, int w, double divergence_px,
                         double separation_px, double exponent, double convergence, double gradient_threshold,
                         float* warped, uint8_t* gap_mask, void* workspace, size_t workspace_bytes, void* stream_) {
    return forward_warp_common(image, depth, n, h, w, divergence_px, separation_px, exponent, convergence, 1,
                               gradient_threshold, warped, gap_mask, workspace, workspace_bytes, (hipStream_t)stream_);
}

size_t cs_grid_warp_workspace_bytes(int n, int h, int w) {
    (void)h; (void)w;
    return n <= 0 ? 0 : stats_bytes(n) + al256((size_t)n * 16);
}
int cs_grid_warp_max_width(int op) {
    if (op == CS_GRID_MASK || op == CS_GRID_STRETCH) return gridwarp_max_width();
    return (op == CS_GRID_WARP || op == CS_GRID_FILL) ? 0x7fffffff : 0;
}

int cs_grid_warp(const float* image, const float* depth, int n, int c, int h, int w, double divergence_px, double separation_px,
                 double exponent, double convergence, int op, int padding, float* warped, uint8_t* mask, void* workspace,
                 size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (op < CS_GRID_WARP || op > CS_GRID_STRETCH) return fail(CS_EINVAL, "cs_grid_warp: unknown operation (CS_GRID_*)");
    if (padding < CS_GRID_PAD_BORDER || padding > CS_GRID_PAD_REFLECTION) return fail(CS_EINVAL, "cs_grid_warp: unknown padding (CS_GRID_PAD_*)");
    if (op != CS_GRID_FILL && padding != CS_GRID_PAD_BORDER) return fail(CS_EINVAL, "cs_grid_warp: only CS_GRID_FILL takes a padding mode");
    if (op == CS_GRID_MASK) warped = nullptr;
    if (op == CS_GRID_WARP) mask = nullptr;
    if (!depth || !workspace || (warped && !image)) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || (warped && c <= 0)) return fail(CS_EINVAL, "non-positive size");
    if (n > 65535) return fail(CS_ELIMIT, "cs_grid_warp: more than 65535 frames in one call");
    if ((size_t)h * w >= (1ull << 31)) return fail(CS_ELIMIT, "cs_grid_warp: frame of 2^31 pixels or more");
    if ((op == CS_GRID_MASK || op == CS_GRID_STRETCH) && w > gridwarp_max_width())
        return fail(CS_ELIMIT, "cs_grid_warp: frame too wide for the LDS-resident row (cs_grid_warp_max_width)");
    if (workspace_bytes < cs_grid_warp_workspace_bytes(n, h, w)) return fail(CS_EWORKSPACE, "workspace too small");
    if (!warped && !mask) return CS_OK;
    uint32_t* stats = (uint32_t*)workspace;
    float* fconst = (float*)((char*)workspace + stats_bytes(n));
    stats_prepass(stats, n, depth, (size_t)h * w, stream, NanInDepth::POISONS);   // (amin / amax of a frame with a NaN are NaN: the frame is flat)
    hipError_t e = launch_gridwarp(image, depth, n, c, h, w, divergence_px, separation_px, exponent, convergence, op, padding,
                                   warped, mask, stats, fconst, stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_grid_warp");
}

int cs_interpolate_fill(const float* image, const uint8_t* mask, int n, int c, int h, int w, float* out, void* stream) {
    if (!image || !mask || !out) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (n > 65535) return fail(CS_ELIMIT, "cs_interpolate_fill: more than 65535 frames in one call");
    if ((size_t)w > (1u << 24)) return fail(CS_ELIMIT, "cs_interpolate_fill: rows of more than 2^24 columns");
    if (image == out) return fail(CS_EINVAL, "cs_interpolate_fill: out must not alias image");
    hipError_t e = launch_interp_fill(image, mask, n, c, h, w, out, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_interpolate_fill");
}

int cs_detect_disocclusions(const float* depth, const float* grid, const float* grid_x_warped, int h, int w, double threshold,
                            uint8_t* out, void* stream) {
    if (!depth || !grid || !grid_x_warped || !out) return fail(CS_EINVAL, "null pointer");
    if (h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (w < 2) return fail(CS_EINVAL, "cs_detect_disocclusions: w >= 2 (the last column takes the step before it)");
    hipError_t e = launch_detect_disocc(depth, grid, grid_x_warped, h, w, threshold, out, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_detect_disocclusions");
}

size_t cs_inpaint_prepare_workspace_bytes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return stats_bytes(n) + 2 * al256(inpaint_prep_bits_bytes(n, h, w));
}
int cs_inpaint_prepare_max_width(void) { return inpaint_prep_max_width(); }

int cs_inpaint_prepare(const float* image, const float* depth, int n, int h, int w, double divergence_px, double threshold,
                       float* warped, float* filled, uint8_t* mask, uint8_t* warped_u8, uint8_t* filled_u8, void* workspace,
                       size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!image || !depth || !workspace) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (n > 65535) return fail(CS_ELIMIT, "cs_inpaint_prepare: more than 65535 frames in one call");
    if ((size_t)h * w >= (1ull << 31)) return fail(CS_ELIMIT, "cs_inpaint_prepare: frame of 2^31 pixels or more");
    if (w > inpaint_prep_max_width())
        return fail(CS_ELIMIT, "cs_inpaint_prepare: frame too wide for the LDS-resident bit row (cs_inpaint_prepare_max_width)");
    if (workspace_bytes < cs_inpaint_prepare_workspace_bytes(n, h, w)) return fail(CS_EWORKSPACE, "workspace too small");
    if (!warped && !filled && !mask && !warped_u8 && !filled_u8) return CS_OK;
    uint32_t* stats = (uint32_t*)workspace;
    const size_t bits = al256(inpaint_prep_bits_bytes(n, h, w));
    uint32_t* nvb = (uint32_t*)((char*)workspace + stats_bytes(n));
    uint32_t* disb = (uint32_t*)((char*)nvb + bits);
    stats_prepass(stats, n, depth, (size_t)h * w, stream, NanInDepth::POISONS);   // (d.min() / d.max() of a frame with a NaN are NaN: the frame is flat)
    hipError_t e = launch_inpaint_prep(image, depth, n, h, w, divergence_px, threshold, warped, filled, mask, warped_u8, filled_u8,
                                       stats, nvb, disb, stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_inpaint_prepare");
}

size_t cs_pil_resize_workspace_bytes(int n, int h, int w, int c, int oh, int ow) {
    if (n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || (c != 1 && c != 3)) return 0;
    if (!pilresize_fits(h, w, oh, ow)) return 0;
    return pilresize_workspace_bytes(n, h, w, c, oh, ow) + 256;
}
int cs_pil_resize_max_taps(void) { return pilresize_max_taps(); }

static bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + nb && pb < pa + na;
}

// ---- the buffer checks that entry points share --------------------------------------------------------------------------------
// some pointer (null ones aside) is off the grid of `elem_bytes`, a power of two
static bool misaligned(size_t elem_bytes, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    return (bits & (elem_bytes - 1)) != 0;
}

struct span { const void* p; size_t bytes; };

// some written region overlaps another one or a read one (a null region overlaps nothing).  An entry point that refuses overlap
// between any two of its buffers, read-only pairs included, passes them all as `outs`.
static bool any_overlap(const span* outs, int n_out, const span* ins, int n_in) {
    for (int i = 0; i < n_out; i++) {
        for (int j = i + 1; j < n_out; j++)
            if (overlaps(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes)) return true;
        for (int j = 0; j < n_in; j++)
            if (overlaps(outs[i].p, outs[i].bytes, ins[j].p, ins[j].bytes)) return true;
    }
    return false;
}

// an entry point's buffers as one table (the depth pre-passes): a null pointer among the first n, one off the grid of `elem_bytes`
static bool any_null(const span* bufs, int n) {
    for (int i = 0; i < n; i++)
        if (!bufs[i].p) return true;
    return false;
}
static bool misaligned(size_t elem_bytes, const span* bufs, int n) {
    uintptr_t bits = 0;
    for (int i = 0; i < n; i++) bits |= (uintptr_t)bufs[i].p;
    return (bits & (elem_bytes - 1)) != 0;
}

int cs_pil_resize(const void* in, int n, int h, int w, int c, int oh, int ow, int flags, uint8_t* out_u8, float* out_f32,
                  size_t f32_row_pitch, void* workspace, size_t workspace_bytes, void* stream) {
    if (!in || !workspace) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0) return fail(CS_EINVAL, "non-positive size");
    if (flags & ~(CS_PIL_IN_F32 | CS_PIL_GRAY | CS_PIL_OUT_PLANAR)) return fail(CS_EINVAL, "cs_pil_resize: unknown flag (CS_PIL_*)");
    if (c != 1 && c != 3) return fail(CS_EINVAL, "cs_pil_resize: 1 or 3 channels (modes L and RGB)");
    if ((flags & CS_PIL_GRAY) && c != 3) return fail(CS_EINVAL, "cs_pil_resize: CS_PIL_GRAY takes 3 channels");
    const int in_f32 = (flags & CS_PIL_IN_F32) != 0, gray = (flags & CS_PIL_GRAY) != 0, planar = (flags & CS_PIL_OUT_PLANAR) != 0;
    const int co = gray ? 1 : c;
    const size_t dense = (size_t)ow * co;
    if (!planar && f32_row_pitch != 0 && f32_row_pitch < dense) return fail(CS_EINVAL, "cs_pil_resize: f32_row_pitch below ow * channels");
    if (in_f32 && ((uintptr_t)in & 3)) return fail(CS_EINVAL, "cs_pil_resize: float32 input needs 4-byte alignment");
    if ((uintptr_t)out_f32 & 3) return fail(CS_EINVAL, "cs_pil_resize: out_f32 needs 4-byte alignment");
    if ((uintptr_t)workspace & 7) return fail(CS_EINVAL, "cs_pil_resize: workspace needs 8-byte alignment");
    if (n > 65535) return fail(CS_ELIMIT, "cs_pil_resize: more than 65535 frames in one call");
    if (h > pilresize_max_size() || w > pilresize_max_size() || oh > pilresize_max_size() || ow > pilresize_max_size())
        return fail(CS_ELIMIT, "cs_pil_resize: a side of more than 65535 samples");
    if (!pilresize_fits(h, w, oh, ow))
        return fail(CS_ELIMIT, "cs_pil_resize: reduction too strong for the LDS-resident input span (cs_pil_resize_max_taps)");
    const size_t pitch = planar ? 0 : (f32_row_pitch ? f32_row_pitch : dense);
    const size_t in_bytes = (size_t)n * h * w * c * (in_f32 ? 4 : 1), u8_bytes = (size_t)n * oh * dense;
    const size_t f32_bytes = planar ? u8_bytes * 4 : ((size_t)n * oh - 1) * pitch * 4 + dense * 4;
    const size_t need = cs_pil_resize_workspace_bytes(n, h, w, c, oh, ow);
    if (overlaps(in, in_bytes, out_u8, u8_bytes) || overlaps(in, in_bytes, out_f32, f32_bytes) ||
        overlaps(out_u8, u8_bytes, out_f32, f32_bytes) || overlaps(workspace, need, in, in_bytes) ||
        overlaps(workspace, need, out_u8, u8_bytes) || overlaps(workspace, need, out_f32, f32_bytes))
        return fail(CS_EINVAL, "cs_pil_resize: in, out_u8, out_f32 and workspace must not overlap");
    if (workspace_bytes < need) return fail(CS_EWORKSPACE, "workspace too small");
    if (!out_u8 && !out_f32) return CS_OK;
    void* ws = (void*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    hipError_t e = launch_pilresize(in, in_f32, gray, n, h, w, c, oh, ow, out_u8, out_f32, planar, pitch, ws, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_pil_resize");
}

size_t cs_gaussian_blur_workspace_bytes(int n, int h, int w, int n_taps) {
    (void)n_taps;
    return (n <= 0 || h <= 0 || w <= 0) ? 0 : al256((size_t)n * h * w * 4);
}
int cs_gaussian_blur_max_taps(void) { return gaussblur_max_taps(); }

int cs_gaussian_blur(int op, const float* depth, const double* taps, int n_taps, double edge_threshold, int n, int h, int w,
                     float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (op < CS_GAUSS_PLAIN || op > CS_GAUSS_RIGHT) return fail(CS_EINVAL, "cs_gaussian_blur: unknown operation (CS_GAUSS_*)");
    if (!depth || !taps || !out || !workspace) return fail(CS_EINVAL, "null pointer");
    if (n_taps <= 0 || (n_taps & 1) == 0) return fail(CS_EINVAL, "cs_gaussian_blur: n_taps must be odd and positive (2 * radius + 1)");
    if (n <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (((uintptr_t)depth & 3) || ((uintptr_t)out & 3) || ((uintptr_t)workspace & 3) || ((uintptr_t)taps & 7))
        return fail(CS_EINVAL, "cs_gaussian_blur: float32 buffers need 4-byte, the taps 8-byte alignment");
    if (out == depth || (void*)out == workspace || (const void*)depth == workspace)
        return fail(CS_EINVAL, "cs_gaussian_blur: depth, out and workspace must not alias");
    if (n_taps > gaussblur_max_taps()) return fail(CS_ELIMIT, "cs_gaussian_blur: more taps than cs_gaussian_blur_max_taps()");
    // one workgroup per 1024 columns of a row / per 256 columns of a 16-row band: grids of fewer than 2^24 workgroups
    if ((size_t)n * h * ((w + 1023) / 1024) >= (1u << 24) || (size_t)n * ((h + 15) / 16) * ((w + 255) / 256) >= (1u << 24))
        return fail(CS_ELIMIT, "cs_gaussian_blur: more than 2^24 workgroups in one call (split the batch)");
    if (workspace_bytes < cs_gaussian_blur_workspace_bytes(n, h, w, n_taps)) return fail(CS_EWORKSPACE, "workspace too small");
    hipError_t e = launch_gaussblur(op, depth, taps, n_taps, edge_threshold, n, h, w, out, (float*)workspace, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_gaussian_blur");
}

int cs_expand_u8(const uint8_t* codes, float* out, size_t count, void* stream) {
    if (!codes || !out) return fail(CS_EINVAL, "null pointer");
    if (((uintptr_t)codes & 3) || ((uintptr_t)out & 15)) return fail(CS_EINVAL, "cs_expand_u8 needs 4-/16-byte aligned buffers");
    hipLaunchKernelGGL(k_expand_u8, dim3(grid_for(count / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, codes, out, count);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_expand_u8");
}


int cs_pack_u8(const float* values, uint8_t* codes, size_t count, int stride, int mode, void* stream) {
    if (!values || !codes) return fail(CS_EINVAL, "null pointer");
    if (stride < 1 || mode < 0 || mode > 1) return fail(CS_EINVAL, "cs_pack_u8: stride >= 1, mode 0 (k / 255 values) or 1 (mask flags)");
    if ((uintptr_t)codes & 3) return fail(CS_EINVAL, "cs_pack_u8 needs a 4-byte aligned code buffer");
    if (count == 0) return CS_OK;
    hipLaunchKernelGGL(k_pack_u8, dim3(grid_for(count / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, values, codes, count, stride, mode);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_pack_u8");
}

int cs_take_f32(const float* values, float* out, size_t count, int stride, void* stream) {
    if (!values || !out) return fail(CS_EINVAL, "null pointer");
    if (stride < 1) return fail(CS_EINVAL, "cs_take_f32: stride >= 1");
    if (count == 0) return CS_OK;
    hipLaunchKernelGGL(k_take_f32, dim3(grid_for(count, 256)), dim3(256), 0, (hipStream_t)stream, values, out, count, stride);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_take_f32");
}

size_t cs_stereo_shift_workspace_bytes(void) { return stats_bytes(1); }

int cs_stereo_shift(const float* input, const float* depth, int b, int c, int h, int w, double scale_factor, int shift_both,
                    double stereo_offset_exponent, float* out, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!input || !depth || !out || !workspace) return fail(CS_EINVAL, "null pointer");
    if (b <= 0 || c <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if ((size_t)w * 4 > 64 * 1024) return fail(CS_ELIMIT, "row too wide for the LDS-resident winner table");
    if (workspace_bytes < cs_stereo_shift_workspace_bytes()) return fail(CS_EWORKSPACE, "workspace too small");
    uint32_t* stats = (uint32_t*)workspace;
    // one "frame" = the whole depth tensor: the reference normalises with its global min / max (stereo_utils.py:36-45)
    const size_t total = (size_t)b * h * w;
    if (total >= (1ull << 31)) return fail(CS_ELIMIT, "depth tensor too large");
    stats_prepass(stats, 1, depth, total, stream, NanInDepth::POISONS);
    const double e = stereo_offset_exponent;
    const int pow_mode = stereo_shift_pow_mode(e);
    const size_t half = (size_t)b * c * h * w;
    const double balance = shift_both ? 0.5 : 0.0;
    for (int eye = 0; eye < 2; eye++) {
        float* dst = out + eye * half;
        if (eye == 0 && !shift_both) {   // left = input (:75-77)
            hipError_t e1 = hipMemcpyAsync(dst, input, half * 4, hipMemcpyDeviceToDevice, stream);
            if (e1 != hipSuccess) return fail_hip(e1, "cs_stereo_shift");
            continue;
        }
        const double sf = eye == 0 ? +1 * scale_factor * balance : -1 * scale_factor * (1 - balance);
        const double scale_px = (sf / 100.0) * (double)w;   // (:54)
        hipLaunchKernelGGL(k_stereo_shift, dim3(h, b), dim3(256), (size_t)w * 4, stream, input, depth, c, h, w, stats,
                           (float)scale_px, scale_px < 0 ? 1 : 0, pow_mode, (float)e, dst);
    }
    hipError_t er = hipGetLastError();
    return er == hipSuccess ? CS_OK : fail_hip(er, "cs_stereo_shift");
}

size_t cs_latent_shift_plan_workspace_bytes(void) { return stats_bytes(1); }

int cs_latent_shift_plan(const float* disp, int b, int h, int w, double scale_factor, double stereo_offset_exponent, int32_t* src_col,
                         void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!disp || !src_col || !workspace) return fail(CS_EINVAL, "null pointer");
    if (b <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (!(scale_factor - scale_factor == 0.0) || !(stereo_offset_exponent - stereo_offset_exponent == 0.0))
        return fail(CS_EINVAL, "cs_latent_shift_plan: scale_factor and stereo_offset_exponent must be finite");
    // the destination table of a row stays within 32 KiB of LDS; the scan costs w * reach reads per row: made for latents
    if (w > LATENT_MAX_WIDTH) return fail(CS_ELIMIT, "cs_latent_shift_plan: rows of more than 8192 columns");
    if (b > 65535) return fail(CS_ELIMIT, "cs_latent_shift_plan: more than 65 535 images in one call");
    const size_t total = (size_t)b * h * w;
    if (total >= (1ull << 31)) return fail(CS_ELIMIT, "depth tensor too large");
    if (workspace_bytes < cs_latent_shift_plan_workspace_bytes()) return fail(CS_EWORKSPACE, "workspace too small");
    // the stats pre-pass of cs_stereo_shift: one "frame" = the whole tensor (reference stereo_utils.py:36-45)
    uint32_t* stats = (uint32_t*)workspace;
    stats_prepass(stats, 1, disp, total, stream, NanInDepth::POISONS);
    const double scale_px = ((-1 * scale_factor) / 100.0) * (double)w;   // the right view with balance 0 (:54, :84-86)
    hipError_t e = launch_latent_shift_plan(disp, b, h, w, stats, scale_px, stereo_offset_exponent, src_col, stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_latent_shift_plan");
}

// ---- the checks the latent loops' entry points share (element size and width limit: cs_latent.h) ----
static bool latent_dtype_ok(int dtype) { return dtype >= CS_LATENT_F32 && dtype <= CS_LATENT_BF16; }

// c1..c4 as the kernels take them
struct coeffs4 {
    double d[4];
    float f[4];
    coeffs4(double c1, double c2, double c3, double c4) : d{c1, c2, c3, c4}, f{(float)c1, (float)c2, (float)c3, (float)c4} {}
};

int cs_latent_shift_apply(const void* left, void* right, const int32_t* src_col, uint8_t* mask, const void* noise, int dtype, int b,
                          int c, int h, int w, int op, void* stream) {
    if (!left || !right || !src_col) return fail(CS_EINVAL, "null pointer");
    if (!mask) return fail(CS_EINVAL, op == CS_LATENT_RESHIFT ? "cs_latent_shift_apply: CS_LATENT_RESHIFT reads the mask CS_LATENT_FIRST stored"
                                                               : "null pointer");
    if (b <= 0 || c <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (!latent_dtype_ok(dtype)) return fail(CS_EINVAL, "cs_latent_shift_apply: unknown dtype (CS_LATENT_F32 / F16 / BF16)");
    if (op != CS_LATENT_FIRST && op != CS_LATENT_RESHIFT) return fail(CS_EINVAL, "cs_latent_shift_apply: unknown op (CS_LATENT_FIRST / RESHIFT)");
    const size_t eb = latent_elem_bytes(dtype), bytes = (size_t)b * c * h * w * eb;
    if (misaligned(eb, {left, right, noise})) return fail(CS_EINVAL, "cs_latent_shift_apply: misaligned tensor");
    if (misaligned(4, {src_col})) return fail(CS_EINVAL, "cs_latent_shift_apply: misaligned src_col");
    const span out = {right, bytes}, ins[2] = {{left, bytes}, {noise, bytes}};
    if (any_overlap(&out, 1, ins, 2)) return fail(CS_EINVAL, "cs_latent_shift_apply: right must not overlap left or noise");
    hipError_t e = launch_latent_shift_apply(left, right, src_col, mask, noise, dtype, b, c, h, w, op, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_latent_shift_apply");
}

int cs_decode_to_codes(const void* image, int dtype, int n, int c, int h, int w, uint8_t* codes_nhwc, void* stream) {
    if (!image || !codes_nhwc) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (!latent_dtype_ok(dtype)) return fail(CS_EINVAL, "cs_decode_to_codes: unknown dtype (CS_LATENT_F32 / F16 / BF16)");
    const size_t eb = latent_elem_bytes(dtype), count = (size_t)n * c * h * w;
    if (misaligned(eb, {image})) return fail(CS_EINVAL, "cs_decode_to_codes: misaligned image");
    const span out = {codes_nhwc, count}, in = {image, count * eb};
    if (any_overlap(&out, 1, &in, 1)) return fail(CS_EINVAL, "cs_decode_to_codes: codes must not overlap image");
    hipError_t e = launch_decode_to_codes(image, dtype, n, c, h, w, codes_nhwc, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_decode_to_codes");
}

// ---- null-text inversion outside the UNet (cs_inversion.hip) ----
static bool finite_d(double x) { return x - x == 0.0; }

// the checks cs_ddim_step and cs_null_loss_grad share; c2 divides under CS_PRED_EPSILON and only multiplies under CS_PRED_V
static const char* step_args_error(int dtype, long long count, double guidance, const double c[4], int prediction) {
    if (count <= 0) return "non-positive count";
    if (!latent_dtype_ok(dtype)) return "unknown dtype (CS_LATENT_F32 / F16 / BF16)";
    if (prediction != CS_PRED_EPSILON && prediction != CS_PRED_V) return "unknown prediction (CS_PRED_EPSILON / CS_PRED_V)";
    if (!finite_d(guidance) || !finite_d(c[0]) || !finite_d(c[1]) || !finite_d(c[2]) || !finite_d(c[3]))
        return "guidance and c1..c4 must be finite";
    if (prediction == CS_PRED_EPSILON && (float)c[1] == 0.0f) return "c2 (the square root of alpha_t) must not be 0";
    return nullptr;
}

// d rec / d e of the step (cs_ddimstep.h), in double from the float32 coefficients
static double step_slope(const float c[4], int prediction) {
    if (prediction == CS_PRED_V) return (double)c[2] * (double)c[1] - (double)c[3] * (double)c[0];
    return (double)c[2] - (double)c[3] * (double)c[0] / (double)c[1];
}

// The four *_pred entry points and their epsilon namesakes are one body each: the namesake passes CS_PRED_EPSILON.
int cs_ddim_step_pred(const void* sample, const void* eps_a, const void* eps_b, void* out, int dtype, long long count, double guidance,
                      double c1, double c2, double c3, double c4, int prediction, void* stream) {
    if (!sample || !eps_a || !out) return fail(CS_EINVAL, "null pointer");
    const coeffs4 c(c1, c2, c3, c4);
    if (const char* msg = step_args_error(dtype, count, guidance, c.d, prediction)) return fail(CS_EINVAL, msg);
    const size_t eb = latent_elem_bytes(dtype), bytes = (size_t)count * eb;
    if (misaligned(eb, {sample, eps_a, eps_b, out})) return fail(CS_EINVAL, "cs_ddim_step: misaligned tensor");
    // out may be sample itself: then sample is no input to keep clear of
    const span o = {out, bytes}, ins[3] = {{out == sample ? nullptr : sample, bytes}, {eps_a, bytes}, {eps_b, bytes}};
    if (any_overlap(&o, 1, ins, 3)) return fail(CS_EINVAL, "cs_ddim_step: out may be sample itself; it must not overlap anything else");
    hipError_t e = launch_ddim_step(sample, eps_a, eps_b, out, dtype, (size_t)count, (float)guidance, c.f, prediction, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_ddim_step");
}

int cs_ddim_step(const void* sample, const void* eps_a, const void* eps_b, void* out, int dtype, long long count, double guidance,
                 double c1, double c2, double c3, double c4, void* stream) {
    return cs_ddim_step_pred(sample, eps_a, eps_b, out, dtype, count, guidance, c1, c2, c3, c4, CS_PRED_EPSILON, stream);
}

size_t cs_null_loss_workspace_bytes(long long count) { return count > 0 ? null_loss_workspace_bytes((size_t)count) : 0; }

int cs_null_loss_grad_pred(const void* eps_uncond, const void* eps_cond, const void* latent_cur, const void* latent_prev, void* rec,
                           float* loss, void* grad, int dtype, long long count, double guidance, double c1, double c2, double c3,
                           double c4, int prediction, void* workspace, size_t workspace_bytes, void* stream) {
    if (!eps_uncond || !eps_cond || !latent_cur || !latent_prev || !rec || !loss || !grad) return fail(CS_EINVAL, "null pointer");
    const coeffs4 cc(c1, c2, c3, c4);
    const float* c = cc.f;
    if (const char* msg = step_args_error(dtype, count, guidance, cc.d, prediction)) return fail(CS_EINVAL, msg);
    if ((unsigned long long)count > null_loss_max_count()) return fail(CS_ELIMIT, "cs_null_loss_grad: too many elements for a 32-bit grid");
    const size_t eb = latent_elem_bytes(dtype), bytes = (size_t)count * eb, need = null_loss_workspace_bytes((size_t)count);
    if (misaligned(eb, {eps_uncond, eps_cond, latent_cur, latent_prev, rec, grad})) return fail(CS_EINVAL, "cs_null_loss_grad: misaligned tensor");
    if (misaligned(4, {loss, workspace})) return fail(CS_EINVAL, "cs_null_loss_grad: misaligned loss or workspace");
    if (need && (!workspace || workspace_bytes < need)) return fail(CS_EWORKSPACE, "workspace too small");
    const span outs[3] = {{rec, bytes}, {grad, bytes}, {loss, 4}};
    const span ins[4] = {{eps_uncond, bytes}, {eps_cond, bytes}, {latent_cur, bytes}, {latent_prev, bytes}};
    for (const span& out : outs)
        if (any_overlap(&out, 1, ins, 4)) return fail(CS_EINVAL, "cs_null_loss_grad: outputs must not overlap inputs");
    if (any_overlap(outs, 3, nullptr, 0)) return fail(CS_EINVAL, "cs_null_loss_grad: outputs must not overlap each other");
    // d loss / d eps_uncond = (2 / n) * (rec - latent_prev) * d rec / d e * d e / d eps_uncond
    const double grad_scale = 2.0 / (double)count * step_slope(c, prediction) * (1.0 - (double)(float)guidance);
    hipError_t e = launch_null_loss_grad(eps_uncond, eps_cond, latent_cur, latent_prev, rec, loss, grad, dtype, (size_t)count,
                                         (float)guidance, c, prediction, grad_scale, workspace, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_null_loss_grad");
}

int cs_null_loss_grad(const void* eps_uncond, const void* eps_cond, const void* latent_cur, const void* latent_prev, void* rec,
                      float* loss, void* grad, int dtype, long long count, double guidance, double c1, double c2, double c3, double c4,
                      void* workspace, size_t workspace_bytes, void* stream) {
    return cs_null_loss_grad_pred(eps_uncond, eps_cond, latent_cur, latent_prev, rec, loss, grad, dtype, count, guidance, c1, c2, c3, c4,
                                  CS_PRED_EPSILON, workspace, workspace_bytes, stream);
}

// the checks and the coefficients cs_adam_step and cs_adam_step_frames share
static const char* adam_args_error(int dtype, double lr, double beta1, double beta2, double eps, int step) {
    if (!latent_dtype_ok(dtype)) return "unknown dtype (CS_LATENT_F32 / F16 / BF16)";
    if (step < 1) return "the step number counts from 1";
    if (!finite_d(lr) || !finite_d(eps) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return "lr and eps must be finite, eps >= 0, betas in [0, 1)";
    return nullptr;
}

struct adam6 {
    float k[6];
    // the bias corrections in double, as torch/optim/adam.py computes them from Python floats
    adam6(double lr, double beta1, double beta2, double eps, int step) {
        const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
        const float v[6] = {(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)sqrt(bc2), (float)eps, (float)(-(lr / bc1))};
        for (int i = 0; i < 6; ++i) k[i] = v[i];
    }
};

static int fail_named(int code, const char* entry, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s: %s", entry, msg);
    return code;
}

int cs_adam_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int dtype, long long count, double lr, double beta1,
                 double beta2, double eps, int step, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(CS_EINVAL, "null pointer");
    if (count <= 0) return fail(CS_EINVAL, "non-positive count");
    if (const char* msg = adam_args_error(dtype, lr, beta1, beta2, eps, step)) return fail_named(CS_EINVAL, "cs_adam_step", msg);
    const size_t eb = latent_elem_bytes(dtype), bytes = (size_t)count * eb;
    if (misaligned(eb, {param, grad, exp_avg, exp_avg_sq})) return fail(CS_EINVAL, "cs_adam_step: misaligned tensor");
    const span outs[3] = {{param, bytes}, {exp_avg, bytes}, {exp_avg_sq, bytes}}, in = {grad, bytes};
    if (any_overlap(outs, 3, &in, 1)) return fail(CS_EINVAL, "cs_adam_step: param, grad, exp_avg and exp_avg_sq must not overlap");
    const adam6 a(lr, beta1, beta2, eps, step);
    hipError_t e = launch_adam_step(param, grad, exp_avg, exp_avg_sq, dtype, (size_t)count, a.k, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_adam_step");
}

// ---- null-text optimisation on F frames at once (cs_inversion_frames.hip) ----
size_t cs_null_loss_frames_workspace_bytes(long long frames, long long per) {
    return frames > 0 && per > 0 ? null_loss_frames_workspace_bytes((size_t)frames, (size_t)per) : 0;
}

static const char* frames_error(long long frames, long long per, int* code) {
    *code = CS_EINVAL;
    if (frames <= 0 || per <= 0) return "non-positive count";
    *code = CS_ELIMIT;
    if ((unsigned long long)frames > null_loss_frames_max()) return "too many frames for the grid's second dimension (65535)";
    return nullptr;
}

int cs_null_loss_grad_frames_pred(const void* eps_uncond, const void* eps_cond, const void* latent_cur, const void* latent_prev, void* rec,
                                  float* loss, void* grad, const uint8_t* active_in, uint8_t* active_out, int dtype, long long frames,
                                  long long per, double guidance, double c1, double c2, double c3, double c4, int prediction,
                                  double threshold, void* workspace, size_t workspace_bytes, void* stream) {
    if (!eps_uncond || !eps_cond || !latent_cur || !latent_prev || !rec || !loss || !grad || !active_in || !active_out)
        return fail(CS_EINVAL, "null pointer");
    const coeffs4 cc(c1, c2, c3, c4);
    const float* c = cc.f;
    int code;
    if (const char* msg = frames_error(frames, per, &code)) return fail_named(code, "cs_null_loss_grad_frames", msg);
    if (const char* msg = step_args_error(dtype, per, guidance, cc.d, prediction)) return fail(CS_EINVAL, msg);
    if ((unsigned long long)per > null_loss_max_count())
        return fail(CS_ELIMIT, "cs_null_loss_grad_frames: too many elements per frame for a 32-bit grid");
    if (active_in == active_out) return fail(CS_EINVAL, "cs_null_loss_grad_frames: active_out must not be active_in");
    if (threshold != threshold) return fail(CS_EINVAL, "cs_null_loss_grad_frames: threshold must not be a NaN");
    const size_t eb = latent_elem_bytes(dtype), bytes = (size_t)frames * (size_t)per * eb;
    const size_t need = null_loss_frames_workspace_bytes((size_t)frames, (size_t)per);
    if (misaligned(eb, {eps_uncond, eps_cond, latent_cur, latent_prev, rec, grad}))
        return fail(CS_EINVAL, "cs_null_loss_grad_frames: misaligned tensor");
    if (misaligned(4, {loss, workspace})) return fail(CS_EINVAL, "cs_null_loss_grad_frames: misaligned loss or workspace");
    if (need && (!workspace || workspace_bytes < need)) return fail(CS_EWORKSPACE, "workspace too small");
    const span outs[4] = {{rec, bytes}, {grad, bytes}, {loss, 4 * (size_t)frames}, {active_out, (size_t)frames}};
    const span ins[5] = {{eps_uncond, bytes}, {eps_cond, bytes}, {latent_cur, bytes}, {latent_prev, bytes}, {active_in, (size_t)frames}};
    for (const span& out : outs)
        if (any_overlap(&out, 1, ins, 5)) return fail(CS_EINVAL, "cs_null_loss_grad_frames: outputs must not overlap inputs");
    if (any_overlap(outs, 4, nullptr, 0)) return fail(CS_EINVAL, "cs_null_loss_grad_frames: outputs must not overlap each other");
    // per frame, as cs_null_loss_grad with count = per
    const double grad_scale = 2.0 / (double)per * step_slope(c, prediction) * (1.0 - (double)(float)guidance);
    hipError_t e = launch_null_loss_grad_frames(eps_uncond, eps_cond, latent_cur, latent_prev, rec, loss, grad, active_in, active_out, dtype,
                                                (size_t)frames, (size_t)per, (float)guidance, c, prediction, grad_scale, threshold, workspace,
                                                (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_null_loss_grad_frames");
}

int cs_null_loss_grad_frames(const void* eps_uncond, const void* eps_cond, const void* latent_cur, const void* latent_prev, void* rec,
                             float* loss, void* grad, const uint8_t* active_in, uint8_t* active_out, int dtype, long long frames,
                             long long per, double guidance, double c1, double c2, double c3, double c4, double threshold,
                             void* workspace, size_t workspace_bytes, void* stream) {
    return cs_null_loss_grad_frames_pred(eps_uncond, eps_cond, latent_cur, latent_prev, rec, loss, grad, active_in, active_out, dtype, frames,
                                         per, guidance, c1, c2, c3, c4, CS_PRED_EPSILON, threshold, workspace, workspace_bytes, stream);
}

int cs_adam_step_frames(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, const uint8_t* active, int dtype, long long frames,
                        long long per, double lr, double beta1, double beta2, double eps, int step, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !active) return fail(CS_EINVAL, "null pointer");
    int code;
    if (const char* msg = frames_error(frames, per, &code)) return fail_named(code, "cs_adam_step_frames", msg);
    if (const char* msg = adam_args_error(dtype, lr, beta1, beta2, eps, step)) return fail_named(CS_EINVAL, "cs_adam_step_frames", msg);
    const size_t eb = latent_elem_bytes(dtype), bytes = (size_t)frames * (size_t)per * eb;
    if (misaligned(eb, {param, grad, exp_avg, exp_avg_sq})) return fail(CS_EINVAL, "cs_adam_step_frames: misaligned tensor");
    const span outs[3] = {{param, bytes}, {exp_avg, bytes}, {exp_avg_sq, bytes}}, ins[2] = {{grad, bytes}, {active, (size_t)frames}};
    if (any_overlap(outs, 3, ins, 2)) return fail(CS_EINVAL, "cs_adam_step_frames: param, grad, exp_avg, exp_avg_sq and active must not overlap");
    const adam6 a(lr, beta1, beta2, eps, step);
    hipError_t e = launch_adam_step_frames(param, grad, exp_avg, exp_avg_sq, active, dtype, (size_t)frames, (size_t)per, a.k,
                                           (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_adam_step_frames");
}

// ---- Fast mode's inpainting loop outside its models (cs_inpaintloop.hip) ----
int cs_inpaint_image_prep(const uint8_t* filled, const uint8_t* mask, int n, int h, int w, int hl, int wl, int dtype, void* img,
                          void* masked, void* x, void* stream) {
    if (!filled || !mask || !img || !masked || !x) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || hl <= 0 || wl <= 0) return fail(CS_EINVAL, "non-positive size");
    if (!latent_dtype_ok(dtype)) return fail(CS_EINVAL, "cs_inpaint_image_prep: unknown dtype (CS_LATENT_F32 / F16 / BF16)");
    const size_t eb = latent_elem_bytes(dtype), pixels = (size_t)n * h * w;
    if (misaligned(eb, {img, masked, x})) return fail(CS_EINVAL, "cs_inpaint_image_prep: misaligned tensor");
    const span outs[3] = {{img, pixels * 3 * eb}, {masked, pixels * 3 * eb}, {x, (size_t)2 * n * 9 * hl * wl * eb}};
    const span ins[2] = {{filled, pixels * 3}, {mask, pixels}};
    if (any_overlap(outs, 3, ins, 2)) return fail(CS_EINVAL, "cs_inpaint_image_prep: img, masked and x must not overlap each other or an input");
    hipError_t e = launch_inpaint_image_prep(filled, mask, n, h, w, hl, wl, dtype, img, masked, x, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_inpaint_image_prep");
}

int cs_inpaint_latent_init(const void* mean_img, const void* mean_masked, int mean_dtype, const void* noise, int dtype, int n, int hl,
                           int wl, double sa, double sb, void* x, void* img_latent, void* decode_in, void* stream) {
    if (!mean_img || !mean_masked || !x || !img_latent) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || hl <= 0 || wl <= 0) return fail(CS_EINVAL, "non-positive size");
    if (!latent_dtype_ok(dtype) || !latent_dtype_ok(mean_dtype))
        return fail(CS_EINVAL, "cs_inpaint_latent_init: unknown dtype or mean_dtype (CS_LATENT_F32 / F16 / BF16)");
    if (!finite_d(sa) || !finite_d(sb)) return fail(CS_EINVAL, "cs_inpaint_latent_init: sa and sb must be finite");
    const size_t eb = latent_elem_bytes(dtype), mb = latent_elem_bytes(mean_dtype), count = (size_t)n * 4 * hl * wl;
    if (misaligned(eb, {noise, x, img_latent, decode_in}) || misaligned(mb, {mean_img, mean_masked}))
        return fail(CS_EINVAL, "cs_inpaint_latent_init: misaligned tensor");
    const span outs[3] = {{x, (size_t)2 * n * 9 * hl * wl * eb}, {img_latent, count * eb}, {decode_in, count * eb}};
    const span ins[3] = {{mean_img, count * mb}, {mean_masked, count * mb}, {noise, count * eb}};
    if (any_overlap(outs, 3, ins, 3)) return fail(CS_EINVAL, "cs_inpaint_latent_init: x, img_latent and decode_in must not overlap each other or an input");
    hipError_t e = launch_inpaint_latent_init(mean_img, mean_masked, mean_dtype, noise, dtype, n, hl, wl, (float)sa, (float)sb, x, img_latent,
                                              decode_in, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_inpaint_latent_init");
}

int cs_inpaint_plms_step(const void* noise_pred, void* x, int dtype, int n, int hl, int wl, int kind, double guidance, double sc, double da,
                         double denom, void* e_out, const void* e1, const void* e2, const void* e3, void* cur_sample, void* decode_in,
                         void* stream) {
    if (!noise_pred || !x) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || hl <= 0 || wl <= 0) return fail(CS_EINVAL, "non-positive size");
    if (!latent_dtype_ok(dtype)) return fail(CS_EINVAL, "cs_inpaint_plms_step: unknown dtype (CS_LATENT_F32 / F16 / BF16)");
    if (kind < CS_PLMS_FIRST || kind > CS_PLMS_ORDER4) return fail(CS_EINVAL, "cs_inpaint_plms_step: unknown kind (CS_PLMS_*)");
    // what the kind reads and writes
    if (kind != CS_PLMS_SECOND && !e_out) return fail(CS_EINVAL, "cs_inpaint_plms_step: null e_out (every kind but CS_PLMS_SECOND keeps its prediction)");
    if (kind <= CS_PLMS_SECOND && !cur_sample) return fail(CS_EINVAL, "cs_inpaint_plms_step: null cur_sample (CS_PLMS_FIRST writes it, CS_PLMS_SECOND reads it)");
    if ((kind >= CS_PLMS_SECOND && !e1) || (kind >= CS_PLMS_ORDER3 && !e2) || (kind >= CS_PLMS_ORDER4 && !e3))
        return fail(CS_EINVAL, "cs_inpaint_plms_step: null history (e1 from CS_PLMS_SECOND, e2 from ORDER3, e3 for ORDER4)");
    if (!finite_d(guidance) || !finite_d(sc) || !finite_d(da) || !finite_d(denom))
        return fail(CS_EINVAL, "cs_inpaint_plms_step: guidance, sc, da and denom must be finite");
    if ((float)denom == 0.0f) return fail(CS_EINVAL, "cs_inpaint_plms_step: denom must not be 0");
    // (a pointer the kind does not use is not passed on, whatever it holds)
    if (kind == CS_PLMS_SECOND) e_out = nullptr;
    if (kind > CS_PLMS_SECOND) cur_sample = nullptr;
    if (kind < CS_PLMS_SECOND) e1 = nullptr;
    if (kind < CS_PLMS_ORDER3) e2 = nullptr;
    if (kind < CS_PLMS_ORDER4) e3 = nullptr;
    const size_t eb = latent_elem_bytes(dtype), bytes = (size_t)n * 4 * hl * wl * eb;
    if (misaligned(eb, {noise_pred, x, e_out, e1, e2, e3, cur_sample, decode_in})) return fail(CS_EINVAL, "cs_inpaint_plms_step: misaligned tensor");
    // cur_sample is written by CS_PLMS_FIRST and read by CS_PLMS_SECOND
    const span outs[4] = {{x, (size_t)2 * n * 9 * hl * wl * eb}, {e_out, bytes}, {decode_in, bytes}, {kind == CS_PLMS_FIRST ? cur_sample : nullptr, bytes}};
    const span ins[5] = {{noise_pred, 2 * bytes}, {e1, bytes}, {e2, bytes}, {e3, bytes}, {kind == CS_PLMS_SECOND ? cur_sample : nullptr, bytes}};
    if (any_overlap(outs, 4, ins, 5))
        return fail(CS_EINVAL, "cs_inpaint_plms_step: x, e_out, cur_sample and decode_in must not overlap each other or an input");
    hipError_t e = launch_inpaint_plms_step(noise_pred, x, dtype, n, hl, wl, kind, (float)guidance, (float)sc, (float)da, (float)denom, e_out,
                                            e1, e2, e3, cur_sample, decode_in, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_inpaint_plms_step");
}

// ---- Fast mode's loop for few-step models (cs_fewstep.hip) ----
static const char* fewstep_args_error(int dtype, int channels, int sampler) {
    if (!latent_dtype_ok(dtype)) return "unknown dtype (CS_LATENT_F32 / F16 / BF16)";
    if (sampler != CS_FEWSTEP_EULER && sampler != CS_FEWSTEP_LCM) return "unknown sampler (CS_FEWSTEP_EULER / CS_FEWSTEP_LCM)";
    if (channels != 4 && channels != 9) return "channels must be 9 (an inpainting UNet) or 4";
    return nullptr;
}

int cs_inpaint_fewstep_init(const void* img_latent, const void* noise, const void* x9, int dtype, int n, int hl, int wl, int channels,
                            int cfg, int sampler, double k0, double k1, void* x, void* state, void* mask_l, void* stream) {
    if (!img_latent || !x) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || hl <= 0 || wl <= 0) return fail(CS_EINVAL, "non-positive size");
    if (const char* msg = fewstep_args_error(dtype, channels, sampler)) return fail_named(CS_EINVAL, "cs_inpaint_fewstep_init", msg);
    if (channels == 4 && (!x9 || !mask_l))
        return fail(CS_EINVAL, "cs_inpaint_fewstep_init: 4 channels take x9 (the mask's source) and mask_l");
    if (sampler == CS_FEWSTEP_EULER && !state) return fail(CS_EINVAL, "cs_inpaint_fewstep_init: null state (CS_FEWSTEP_EULER keeps the un-scaled sample)");
    if (!finite_d(k0) || !finite_d(k1)) return fail(CS_EINVAL, "cs_inpaint_fewstep_init: k0 and k1 must be finite");
    if (noise && sampler == CS_FEWSTEP_EULER && (float)k1 == 0.0f) return fail(CS_EINVAL, "cs_inpaint_fewstep_init: k1 (the input scale) must not be 0");
    if (channels == 9) x9 = nullptr, mask_l = nullptr;   // (a pointer the layout does not use is not passed on)
    const int halves = cfg ? 2 : 1;
    const size_t eb = latent_elem_bytes(dtype), plane = (size_t)n * hl * wl * eb, bytes = 4 * plane;
    if (misaligned(eb, {img_latent, noise, x9, x, state, mask_l})) return fail(CS_EINVAL, "cs_inpaint_fewstep_init: misaligned tensor");
    const span outs[3] = {{x, (size_t)halves * channels * plane}, {state, bytes}, {mask_l, plane}};
    const span ins[3] = {{img_latent, bytes}, {noise, bytes}, {x9, 18 * plane}};
    if (any_overlap(outs, 3, ins, 3)) return fail(CS_EINVAL, "cs_inpaint_fewstep_init: x, state and mask_l must not overlap each other or an input");
    hipError_t e = launch_inpaint_fewstep_init(img_latent, noise, x9, dtype, n, hl, wl, channels, halves, sampler, (float)k0, (float)k1, x, state,
                                               mask_l, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_inpaint_fewstep_init");
}

int cs_inpaint_fewstep_step(const void* noise_pred, void* x, int dtype, int n, int hl, int wl, int channels, int sampler, int cfg, int last,
                            double guidance, double k0, double k1, double k2, double k3, double k4, double k5, void* state,
                            const void* step_noise, const void* img_latent, const void* noise0, const void* mask_l, void* decode_in,
                            void* stream) {
    if (!noise_pred || !x) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || hl <= 0 || wl <= 0) return fail(CS_EINVAL, "non-positive size");
    if (const char* msg = fewstep_args_error(dtype, channels, sampler)) return fail_named(CS_EINVAL, "cs_inpaint_fewstep_step", msg);
    // what the sampler and the layout read and write
    if (sampler == CS_FEWSTEP_EULER && !state) return fail(CS_EINVAL, "cs_inpaint_fewstep_step: null state (CS_FEWSTEP_EULER reads and writes the un-scaled sample)");
    if (sampler == CS_FEWSTEP_LCM && !last && !step_noise)
        return fail(CS_EINVAL, "cs_inpaint_fewstep_step: null step_noise (every CS_FEWSTEP_LCM step but the last adds fresh noise)");
    if (channels == 4 && (!img_latent || !mask_l || (!last && !noise0)))
        return fail(CS_EINVAL, "cs_inpaint_fewstep_step: 4 channels take img_latent, mask_l and, before the last step, noise0 (the blend)");
    const double kd[6] = {k0, k1, k2, k3, k4, k5};
    for (double v : kd)
        if (!finite_d(v)) return fail(CS_EINVAL, "cs_inpaint_fewstep_step: guidance and k0..k5 must be finite");
    if (!finite_d(guidance)) return fail(CS_EINVAL, "cs_inpaint_fewstep_step: guidance and k0..k5 must be finite");
    if ((float)k1 == 0.0f) return fail(CS_EINVAL, "cs_inpaint_fewstep_step: k1 (Euler: the input scale, LCM: sqrt(a_t)) must not be 0");
    // (a pointer the sampler, the layout or the step does not use is not passed on, whatever it holds)
    if (sampler == CS_FEWSTEP_LCM) state = nullptr;
    if (sampler == CS_FEWSTEP_EULER || last) step_noise = nullptr;
    if (channels == 9) img_latent = nullptr, noise0 = nullptr, mask_l = nullptr;
    if (last) noise0 = nullptr;
    const int halves = cfg ? 2 : 1;
    const size_t eb = latent_elem_bytes(dtype), plane = (size_t)n * hl * wl * eb, bytes = 4 * plane;
    if (misaligned(eb, {noise_pred, x, state, step_noise, img_latent, noise0, mask_l, decode_in}))
        return fail(CS_EINVAL, "cs_inpaint_fewstep_step: misaligned tensor");
    const span outs[3] = {{x, (size_t)halves * channels * plane}, {state, bytes}, {decode_in, bytes}};
    const span ins[5] = {{noise_pred, halves * bytes}, {step_noise, bytes}, {img_latent, bytes}, {noise0, bytes}, {mask_l, plane}};
    if (any_overlap(outs, 3, ins, 5))
        return fail(CS_EINVAL, "cs_inpaint_fewstep_step: x, state and decode_in must not overlap each other or an input");
    const float kf[6] = {(float)k0, (float)k1, (float)k2, (float)k3, (float)k4, (float)k5};
    hipError_t e = launch_inpaint_fewstep_step(noise_pred, x, dtype, n, hl, wl, channels, sampler, cfg ? 1 : 0, last ? 1 : 0, (float)guidance, kf,
                                               state, step_noise, img_latent, noise0, mask_l, decode_in, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_inpaint_fewstep_step");
}

// ---- Standard mode between two UNet calls (cs_standardloop.hip) ----
int cs_standard_step_pred(void* x, const void* noise_pred, int dtype, int b, int c, int h, int w, double guidance, double c1, double c2,
                          double c3, double c4, int prediction, int op, const int32_t* src_col, uint8_t* mask, const void* noise,
                          void* stream) {
    if (!x || !noise_pred) return fail(CS_EINVAL, "null pointer");
    if (b <= 0 || c <= 0 || h <= 0 || w <= 0) return fail(CS_EINVAL, "non-positive size");
    if (op < CS_STANDARD_NONE || op > CS_STANDARD_RESHIFT) return fail(CS_EINVAL, "cs_standard_step: unknown op (CS_STANDARD_NONE / FIRST / RESHIFT)");
    const coeffs4 cc(c1, c2, c3, c4);
    if (const char* msg = step_args_error(dtype, 1, guidance, cc.d, prediction)) return fail(CS_EINVAL, msg);
    if (op != CS_STANDARD_NONE && (!src_col || !mask)) return fail(CS_EINVAL, "cs_standard_step: a shift op takes src_col and mask");
    if (noise && op != CS_STANDARD_FIRST) return fail(CS_EINVAL, "cs_standard_step: noise goes with CS_STANDARD_FIRST only");
    if (w > LATENT_MAX_WIDTH) return fail(CS_ELIMIT, "cs_standard_step: rows of more than 8192 columns");
    if ((size_t)b * h > 0x7fffffffull || (size_t)c * w > 0x7fffffffull) return fail(CS_ELIMIT, "cs_standard_step: b * h or c * w beyond 2^31 - 1");
    if (op == CS_STANDARD_NONE) src_col = nullptr, mask = nullptr;   // (a pointer the op does not use is not passed on)
    const size_t eb = latent_elem_bytes(dtype), pixels = (size_t)b * h * w, view_bytes = pixels * c * eb;
    if (misaligned(eb, {x, noise_pred, noise})) return fail(CS_EINVAL, "cs_standard_step: misaligned tensor");
    if (misaligned(4, {src_col})) return fail(CS_EINVAL, "cs_standard_step: misaligned src_col");
    const span outs[2] = {{x, 4 * view_bytes}, {mask, pixels}};
    const span ins[3] = {{noise_pred, 4 * view_bytes}, {src_col, pixels * 4}, {noise, view_bytes}};
    if (any_overlap(outs, 2, ins, 3)) return fail(CS_EINVAL, "cs_standard_step: x and mask must not overlap each other or an input");
    hipError_t e = launch_standard_step(x, noise_pred, dtype, b, c, h, w, (float)guidance, cc.f, prediction, op, src_col, mask, noise,
                                        (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_standard_step");
}

int cs_standard_step(void* x, const void* noise_pred, int dtype, int b, int c, int h, int w, double guidance, double c1, double c2,
                     double c3, double c4, int op, const int32_t* src_col, uint8_t* mask, const void* noise, void* stream) {
    return cs_standard_step_pred(x, noise_pred, dtype, b, c, h, w, guidance, c1, c2, c3, c4, CS_PRED_EPSILON, op, src_col, mask, noise, stream);
}

int cs_stereo_attention_max_head_dim(void) { return stereo_attention_max_head_dim(); }

// The argument checks of the six attention entry points, in one order: null pointers, dtype, sizes, mode, scale, head dimension,
// then alignment and the index limits (the stereo forwards check alignment first, the differentiable family -- fwd_lse and bwd,
// SELF mode with c = s = 1 -- the limits), the workspace, and last that no written region overlaps an earlier one.
// elem: bytes per element, 4 (float32; dtype is not looked at) or 2 (dtype: enum cs_attn_dtype); a row of d elements is a whole
// number of 16-byte chunks.  p[0 .. n_in) are read, p[n_in .. n_all) written; a region's size follows from the tensor it is shaped
// like (ATTN_W: the backward's workspace, of which the caller holds workspace_bytes).
enum attn_shape { ATTN_Q, ATTN_K, ATTN_LSE, ATTN_W };   // [(c s b h)][n][d], [(c s b h)][n_k][d], float32 [(b h)][n], workspace
struct attn_ptr { const void* p; attn_shape shape; };

static int attn_fail(int code, const char* fn, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg);
    return code;
}

static int attn_check(const char* fn, int elem, int dtype, bool grad, int c, int s, int b, int h, int n, int n_k, int d, double scale,
                      int mode, const attn_ptr* p, int n_in, int n_all, size_t workspace_bytes) {
    for (int i = 0; i < n_all; i++)
        if (!p[i].p) return fail(CS_EINVAL, "null pointer");
    if (elem == 2 && dtype != CS_ATTN_F16 && dtype != CS_ATTN_BF16) return attn_fail(CS_EINVAL, fn, "unknown dtype (CS_ATTN_F16, CS_ATTN_BF16)");
    if (c <= 0 || s <= 0 || b <= 0 || h <= 0 || n <= 0 || n_k <= 0 || d <= 0) return fail(CS_EINVAL, "non-positive size");
    if (mode < CS_ATTN_SELF || mode > CS_ATTN_BI) return attn_fail(CS_EINVAL, fn, "unknown mode (CS_ATTN_*)");
    if (mode != CS_ATTN_SELF && (s != 2 || n_k != n))
        return attn_fail(CS_EINVAL, fn, "CS_ATTN_UNI / CS_ATTN_BI take two views (s = 2) with n_k = n");
    if (!finite_d(scale)) return attn_fail(CS_EINVAL, fn, "scale must be finite");
    if ((d & (16 / elem - 1)) || d > stereo_attention_max_head_dim())
        return attn_fail(CS_ELIMIT, fn, elem == 2 ? "float16 / bfloat16 head dimension must be a multiple of 8 up to cs_stereo_attention_max_head_dim()"
                                                  : "head dimension must be a multiple of 4 up to cs_stereo_attention_max_head_dim()");
    // one workgroup per 32 * waves queries of a (c, s, b, h) (backward: or keys); token and key indices in 32-bit ints
    const long long bhn = (long long)c * s * b * h;
    const long long tiles = grad ? (n > n_k ? n : n_k) / 32 + 1 : (n + 31) / 32;
    const bool limit = n > (1 << 24) || n_k > (1 << 24) || bhn >= (1ll << 31) || bhn * tiles >= (1ll << 31);
    bool aligned = true;
    for (int i = 0; i < n_all; i++) aligned = aligned && !((uintptr_t)p[i].p & 15);
    if (!aligned && !grad) return attn_fail(CS_EINVAL, fn, "every pointer needs 16-byte alignment");
    if (limit) return attn_fail(CS_ELIMIT, fn, "more than 2^24 tokens per view or 2^31 workgroups in one call");
    if (!aligned) return attn_fail(CS_EINVAL, fn, "every pointer needs 16-byte alignment");
    const size_t need = attention_bwd_workspace_bytes(b, h, n, n_k, d);
    const size_t shape_bytes[4] = {(size_t)bhn * n * d * elem, (size_t)bhn * n_k * d * elem, (size_t)bhn * n * 4, need};
    for (int i = 0; i < n_all; i++)
        if (p[i].shape == ATTN_W && workspace_bytes < need) {
            snprintf(g_err, sizeof(g_err), "%s: workspace too small (%s_workspace_bytes)", fn, fn);
            return CS_EWORKSPACE;
        }
    for (int w = n_in; w < n_all; w++)
        for (int i = 0; i < w; i++)
            if (overlaps(p[w].p, shape_bytes[p[w].shape], p[i].p, shape_bytes[p[i].shape]))
                return attn_fail(CS_EINVAL, fn, "a written tensor (or the workspace) must not overlap an input or another written one");
    return CS_OK;
}

int cs_stereo_attention(const float* q, const float* k, const float* v, float* out, int c, int s, int b, int h, int n, int n_k,
                        int d, double scale, int mode, void* stream) {
    const attn_ptr p[4] = {{q, ATTN_Q}, {k, ATTN_K}, {v, ATTN_K}, {out, ATTN_Q}};
    if (int rc = attn_check("cs_stereo_attention", 4, 0, false, c, s, b, h, n, n_k, d, scale, mode, p, 3, 4, 0)) return rc;
    hipError_t e = launch_stereo_attention(q, k, v, out, c, s, b, h, n, n_k, d, (float)scale, mode, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_stereo_attention");
}

int cs_stereo_attention_half(const void* q, const void* k, const void* v, void* out, int dtype, int c, int s, int b, int h, int n,
                             int n_k, int d, double scale, int mode, void* stream) {
    const attn_ptr p[4] = {{q, ATTN_Q}, {k, ATTN_K}, {v, ATTN_K}, {out, ATTN_Q}};
    if (int rc = attn_check("cs_stereo_attention_half", 2, dtype, false, c, s, b, h, n, n_k, d, scale, mode, p, 3, 4, 0)) return rc;
    hipError_t e = launch_stereo_attention_half(q, k, v, out, dtype, c, s, b, h, n, n_k, d, (float)scale, mode, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_stereo_attention_half");
}

int cs_attention_fwd_lse(const float* q, const float* k, const float* v, float* out, float* lse, int b, int h, int n, int n_k, int d,
                         double scale, void* stream) {
    const attn_ptr p[5] = {{q, ATTN_Q}, {k, ATTN_K}, {v, ATTN_K}, {out, ATTN_Q}, {lse, ATTN_LSE}};
    if (int rc = attn_check("cs_attention_fwd_lse", 4, 0, true, 1, 1, b, h, n, n_k, d, scale, CS_ATTN_SELF, p, 3, 5, 0)) return rc;
    hipError_t e = launch_attention_fwd_lse(q, k, v, out, lse, b, h, n, n_k, d, (float)scale, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_attention_fwd_lse");
}

int cs_attention_half_fwd_lse(const void* q, const void* k, const void* v, void* out, float* lse, int dtype, int b, int h, int n, int n_k,
                              int d, double scale, void* stream) {
    const attn_ptr p[5] = {{q, ATTN_Q}, {k, ATTN_K}, {v, ATTN_K}, {out, ATTN_Q}, {lse, ATTN_LSE}};
    if (int rc = attn_check("cs_attention_half_fwd_lse", 2, dtype, true, 1, 1, b, h, n, n_k, d, scale, CS_ATTN_SELF, p, 3, 5, 0)) return rc;
    hipError_t e = launch_attention_half_fwd_lse(q, k, v, out, lse, dtype, b, h, n, n_k, d, (float)scale, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_attention_half_fwd_lse");
}

// one workspace rule for every dtype: delta, one float32 per query
size_t cs_attention_bwd_workspace_bytes(int b, int h, int n, int n_k, int d) { return attention_bwd_workspace_bytes(b, h, n, n_k, d); }
size_t cs_attention_half_bwd_workspace_bytes(int b, int h, int n, int n_k, int d) { return attention_bwd_workspace_bytes(b, h, n, n_k, d); }

int cs_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* d_out, float* dq,
                     float* dk, float* dv, int b, int h, int n, int n_k, int d, double scale, void* workspace, size_t workspace_bytes,
                     void* stream) {
    const attn_ptr p[10] = {{q, ATTN_Q}, {k, ATTN_K}, {v, ATTN_K}, {out, ATTN_Q}, {lse, ATTN_LSE}, {d_out, ATTN_Q},
                            {dq, ATTN_Q}, {dk, ATTN_K}, {dv, ATTN_K}, {workspace, ATTN_W}};
    if (int rc = attn_check("cs_attention_bwd", 4, 0, true, 1, 1, b, h, n, n_k, d, scale, CS_ATTN_SELF, p, 6, 10, workspace_bytes)) return rc;
    hipError_t e = launch_attention_bwd(q, k, v, out, lse, d_out, dq, dk, dv, b, h, n, n_k, d, (float)scale, workspace, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_attention_bwd");
}

int cs_attention_half_bwd(const void* q, const void* k, const void* v, const void* out, const float* lse, const void* d_out, void* dq,
                          void* dk, void* dv, int dtype, int b, int h, int n, int n_k, int d, double scale, void* workspace,
                          size_t workspace_bytes, void* stream) {
    const attn_ptr p[10] = {{q, ATTN_Q}, {k, ATTN_K}, {v, ATTN_K}, {out, ATTN_Q}, {lse, ATTN_LSE}, {d_out, ATTN_Q},
                            {dq, ATTN_Q}, {dk, ATTN_K}, {dv, ATTN_K}, {workspace, ATTN_W}};
    if (int rc = attn_check("cs_attention_half_bwd", 2, dtype, true, 1, 1, b, h, n, n_k, d, scale, CS_ATTN_SELF, p, 6, 10, workspace_bytes))
        return rc;
    hipError_t e = launch_attention_half_bwd(q, k, v, out, lse, d_out, dq, dk, dv, dtype, b, h, n, n_k, d, (float)scale, workspace,
                                             (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_attention_half_bwd");
}

// ---- the depth pre-passes (cs_temporal_depth, cs_depth_range, cs_guided_depth_*, cs_depth_dilate) -------------------------------
// Each entry point lists its buffers once, in a span table, and checks null pointers, alignment and overlap off it.  The kernels
// take every buffer through a pointer they treat as distinct, so any two overlapping ones are refused, read-only pairs included.
// (The table is made before the sizes are checked; a refused call never uses its byte counts.)

// the limits they share: the frames are the grid's second dimension, a frame's pixel index fits 31 bits
static int depth_limits(const char* entry, int n, int h, int w) {
    if (n > 65535) return fail_named(CS_ELIMIT, entry, "more than 65535 frames in one call");
    if ((size_t)h * w >= (1ull << 31)) return fail_named(CS_ELIMIT, entry, "frame of 2^31 pixels or more");
    return CS_OK;
}

size_t cs_temporal_depth_workspace_bytes(int n, int h, int w, int c) {
    return (n <= 0 || h <= 0 || w <= 0 || c <= 0) ? 0 : temporal_workspace_bytes(n, h, w);
}

int cs_temporal_depth(const float* depth, int n, int h, int w, int c, double alpha, double motion_threshold, double cut_threshold,
                      float* state_prev_raw, float* state_prev, int32_t* state_valid, float* out, float* m_out, int32_t* cut_out,
                      void* workspace, size_t workspace_bytes, void* stream) {
    const size_t frame = (size_t)h * w * 4, px = (size_t)n * h * w, need = cs_temporal_depth_workspace_bytes(n, h, w, c);
    const span buf[8] = {{depth, px * c * 4}, {out, px * 4}, {state_prev_raw, frame}, {state_prev, frame}, {state_valid, 4},
                         {m_out, (size_t)n * 4}, {cut_out, (size_t)n * 4}, {workspace, need}};
    if (any_null(buf, 8)) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return fail(CS_EINVAL, "non-positive size");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(CS_EINVAL, "cs_temporal_depth: alpha must lie in [0, 1]");
    if (!(motion_threshold >= 0.0)) return fail(CS_EINVAL, "cs_temporal_depth: motion_threshold must be >= 0 (+inf allowed)");
    if (!(cut_threshold >= 0.0)) return fail(CS_EINVAL, "cs_temporal_depth: cut_threshold must be >= 0 (+inf allowed)");
    if (misaligned(4, buf, 8)) return fail(CS_EINVAL, "cs_temporal_depth: every buffer needs 4-byte alignment");
    if (int rc = depth_limits("cs_temporal_depth", n, h, w)) return rc;
    if (any_overlap(buf, 8, nullptr, 0))
        return fail(CS_EINVAL, "cs_temporal_depth: depth, out, the state arrays, m_out, cut_out and workspace must not overlap");
    if (workspace_bytes < need) return fail(CS_EWORKSPACE, "workspace too small");
    hipError_t e = launch_temporal(depth, n, h, w, c, (float)alpha, (float)motion_threshold, (float)cut_threshold, state_prev_raw,
                                   state_prev, state_valid, out, m_out, cut_out, (float*)workspace, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_temporal_depth");
}

size_t cs_motion_depth_workspace_bytes(int n, int h, int w, int c, int search_range) {
    return (n <= 0 || h <= 0 || w <= 0 || c <= 0 || motion_args_error(search_range, 0, 0)) ? 0 : motion_workspace_bytes(n, h, w);
}

int cs_motion_depth(const float* depth, const float* guide, int n, int h, int w, int c, double alpha, double motion_threshold,
                    double cut_threshold, int search_range, int smoothness, int match_threshold, float* state_prev_raw,
                    float* state_prev, uint8_t* state_prev_luma, int32_t* state_valid, float* out, float* m_out, int32_t* cut_out,
                    int8_t* vec_out, int32_t* sad_out, uint8_t* matched_out, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t frame = (size_t)h * w, px = (size_t)n * frame, need = cs_motion_depth_workspace_bytes(n, h, w, c, search_range);
    const size_t blocks = (size_t)n * motion_blocks(h) * motion_blocks(w);
    // (the ten buffers of 4-byte elements first: the three of bytes behind them lie on every grid)
    const span buf[13] = {{depth, px * c * 4}, {guide, px * 3 * 4}, {out, px * 4}, {state_prev_raw, frame * 4}, {state_prev, frame * 4},
                          {state_valid, 4}, {m_out, (size_t)n * 4}, {cut_out, (size_t)n * 4}, {sad_out, blocks * 4}, {workspace, need},
                          {state_prev_luma, frame}, {vec_out, blocks * 2}, {matched_out, blocks}};
    if (any_null(buf, 13)) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return fail(CS_EINVAL, "non-positive size");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(CS_EINVAL, "cs_motion_depth: alpha must lie in [0, 1]");
    if (!(motion_threshold >= 0.0)) return fail(CS_EINVAL, "cs_motion_depth: motion_threshold must be >= 0 (+inf allowed)");
    if (!(cut_threshold >= 0.0)) return fail(CS_EINVAL, "cs_motion_depth: cut_threshold must be >= 0 (+inf allowed)");
    if (const char* msg = motion_args_error(search_range, smoothness, match_threshold)) return fail_named(CS_EINVAL, "cs_motion_depth", msg);
    if (misaligned(4, buf, 10)) return fail(CS_EINVAL, "cs_motion_depth: every buffer of 4-byte elements needs 4-byte alignment");
    if (int rc = depth_limits("cs_motion_depth", n, h, w)) return rc;
    if (any_overlap(buf, 13, nullptr, 0))
        return fail(CS_EINVAL, "cs_motion_depth: depth, guide, out, the state arrays, the per-frame and per-block outputs and workspace must not overlap");
    if (workspace_bytes < need) return fail(CS_EWORKSPACE, "workspace too small");
    hipError_t e = launch_motion_depth(depth, guide, n, h, w, c, (float)alpha, (float)motion_threshold, (float)cut_threshold, search_range,
                                       smoothness, match_threshold, state_prev_raw, state_prev, state_prev_luma, state_valid, out, m_out,
                                       cut_out, vec_out, sad_out, matched_out, workspace, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_motion_depth");
}

size_t cs_motion_depth_pyramid_workspace_bytes(int n, int h, int w, int c, int search_range) {
    return (n <= 0 || h <= 0 || w <= 0 || c <= 0 || pyramid_args_error(search_range, 0, 0)) ? 0 : pyramid_workspace_bytes(n, h, w);
}

int cs_motion_depth_pyramid(const float* depth, const float* guide, int n, int h, int w, int c, double alpha, double motion_threshold,
                            double cut_threshold, int search_range, int smoothness, int match_threshold, float* state_prev_raw,
                            float* state_prev, uint8_t* state_prev_luma, int32_t* state_valid, float* out, float* m_out, int32_t* cut_out,
                            int8_t* vec_out, int32_t* sad_out, uint8_t* matched_out, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t frame = (size_t)h * w, px = (size_t)n * frame, need = cs_motion_depth_pyramid_workspace_bytes(n, h, w, c, search_range);
    const size_t blocks = (size_t)n * motion_blocks(h) * motion_blocks(w);
    // (cs_motion_depth's table: the ten buffers of 4-byte elements first)
    const span buf[13] = {{depth, px * c * 4}, {guide, px * 3 * 4}, {out, px * 4}, {state_prev_raw, frame * 4}, {state_prev, frame * 4},
                          {state_valid, 4}, {m_out, (size_t)n * 4}, {cut_out, (size_t)n * 4}, {sad_out, blocks * 4}, {workspace, need},
                          {state_prev_luma, frame}, {vec_out, blocks * 2}, {matched_out, blocks}};
    if (any_null(buf, 13)) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return fail(CS_EINVAL, "non-positive size");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(CS_EINVAL, "cs_motion_depth_pyramid: alpha must lie in [0, 1]");
    if (!(motion_threshold >= 0.0)) return fail(CS_EINVAL, "cs_motion_depth_pyramid: motion_threshold must be >= 0 (+inf allowed)");
    if (!(cut_threshold >= 0.0)) return fail(CS_EINVAL, "cs_motion_depth_pyramid: cut_threshold must be >= 0 (+inf allowed)");
    if (const char* msg = pyramid_args_error(search_range, smoothness, match_threshold)) return fail_named(CS_EINVAL, "cs_motion_depth_pyramid", msg);
    if (misaligned(4, buf, 10)) return fail(CS_EINVAL, "cs_motion_depth_pyramid: every buffer of 4-byte elements needs 4-byte alignment");
    if (int rc = depth_limits("cs_motion_depth_pyramid", n, h, w)) return rc;
    if (any_overlap(buf, 13, nullptr, 0))
        return fail(CS_EINVAL, "cs_motion_depth_pyramid: depth, guide, out, the state arrays, the per-frame and per-block outputs and workspace must not overlap");
    if (workspace_bytes < need) return fail(CS_EWORKSPACE, "workspace too small");
    hipError_t e = launch_motion_depth_pyramid(depth, guide, n, h, w, c, (float)alpha, (float)motion_threshold, (float)cut_threshold,
                                               search_range, smoothness, match_threshold, state_prev_raw, state_prev, state_prev_luma,
                                               state_valid, out, m_out, cut_out, vec_out, sad_out, matched_out, workspace, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_motion_depth_pyramid");
}

size_t cs_depth_range_workspace_bytes(int n, int h, int w, int c) {
    return (n <= 0 || h <= 0 || w <= 0 || c <= 0) ? 0 : range_workspace_bytes(n);
}

int cs_depth_range(const float* depth, int n, int h, int w, int c, int rank_lo, int rank_hi, double beta, int normalize,
                   const int32_t* cut_or_null, float* state_lo, float* state_hi, int32_t* state_valid, float* out, float* lo_out,
                   float* hi_out, float* raw_lo_out, float* raw_hi_out, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t px = (size_t)n * h * w, per_frame = (size_t)n * 4, need = cs_depth_range_workspace_bytes(n, h, w, c);
    // (cut stands last: it may be absent, which is no null pointer, and a null region overlaps nothing)
    const span buf[11] = {{depth, px * c * 4}, {out, px * 4}, {state_lo, 4}, {state_hi, 4}, {state_valid, 4}, {lo_out, per_frame},
                          {hi_out, per_frame}, {raw_lo_out, per_frame}, {raw_hi_out, per_frame}, {workspace, need},
                          {cut_or_null, per_frame}};
    if (any_null(buf, 10)) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return fail(CS_EINVAL, "non-positive size");
    if (int rc = depth_limits("cs_depth_range", n, h, w)) return rc;
    if (rank_lo < 0 || rank_lo > rank_hi || (size_t)rank_hi >= (size_t)h * w)
        return fail(CS_EINVAL, "cs_depth_range: the ranks must satisfy 0 <= rank_lo <= rank_hi < h * w");
    if (!(beta >= 0.0 && beta <= 1.0)) return fail(CS_EINVAL, "cs_depth_range: beta must lie in [0, 1]");
    if (misaligned(4, buf, 11)) return fail(CS_EINVAL, "cs_depth_range: every buffer needs 4-byte alignment");
    if (any_overlap(buf, 11, nullptr, 0))
        return fail(CS_EINVAL, "cs_depth_range: depth, out, the state words, the four bound arrays, cut and workspace must not overlap");
    if (workspace_bytes < need) return fail(CS_EWORKSPACE, "workspace too small");
    hipError_t e = launch_depth_range(depth, n, h, w, c, rank_lo, rank_hi, (float)beta, normalize != 0, cut_or_null, state_lo, state_hi,
                                      state_valid, out, lo_out, hi_out, raw_lo_out, raw_hi_out, workspace, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_depth_range");
}

static int guided_geometry(int h, int w, int dh, int dw, int radius) {
    if (h <= 0 || w <= 0 || dh <= 0 || dw <= 0) return fail(CS_EINVAL, "non-positive size");
    if (radius < 1 || radius > 3) return fail(CS_EINVAL, "cs_guided_depth: the radius must be 1, 2 or 3");
    if (dh > h || dw > w) return fail(CS_ELIMIT, "cs_guided_depth: the depth map is larger than the image");
    return depth_limits("cs_guided_depth", 1, h, w);   // (the frame's limit; the geometry has no frame count)
}

size_t cs_guided_depth_plan_bytes(int h, int w, int dh, int dw, int radius) {
    return (h <= 0 || w <= 0 || dh <= 0 || dw <= 0 || radius < 1 || radius > 3) ? 0 : guided_plan_bytes(h, w, dh, dw, radius);
}

int cs_guided_depth_plan(int h, int w, int dh, int dw, int radius, double sigma_s, double sigma_r, void* plan, size_t plan_bytes,
                         void* stream) {
    if (!plan) return fail(CS_EINVAL, "null pointer");
    if (int rc = guided_geometry(h, w, dh, dw, radius)) return rc;
    if (!(sigma_s > 0.0) || !(sigma_r > 0.0)) return fail(CS_EINVAL, "cs_guided_depth_plan: sigma_s and sigma_r must be positive");
    if ((uintptr_t)plan & 3) return fail(CS_EINVAL, "cs_guided_depth_plan: every buffer needs 4-byte alignment");
    if (plan_bytes < guided_plan_bytes(h, w, dh, dw, radius)) return fail(CS_EWORKSPACE, "plan buffer too small");
    hipError_t e = launch_guided_plan(h, w, dh, dw, radius, sigma_s, sigma_r, plan, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_guided_depth_plan");
}

int cs_guided_depth_apply(const float* image, const float* depth, int n, int h, int w, int dh, int dw, int c, int radius, const void* plan,
                          size_t plan_bytes, float* out, void* stream) {
    const size_t px = (size_t)n * h * w, need = cs_guided_depth_plan_bytes(h, w, dh, dw, radius);
    const span buf[4] = {{image, px * 3 * 4}, {depth, (size_t)n * dh * dw * c * 4}, {plan, need}, {out, px * 4}};
    if (any_null(buf, 4)) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || c <= 0) return fail(CS_EINVAL, "non-positive size");
    if (int rc = guided_geometry(h, w, dh, dw, radius)) return rc;
    if (int rc = depth_limits("cs_guided_depth_apply", n, h, w)) return rc;
    if (misaligned(4, buf, 4)) return fail(CS_EINVAL, "cs_guided_depth_apply: every buffer needs 4-byte alignment");
    if (any_overlap(buf, 4, nullptr, 0)) return fail(CS_EINVAL, "cs_guided_depth_apply: image, depth, plan and out must not overlap");
    if (plan_bytes < need) return fail(CS_EWORKSPACE, "plan buffer too small");
    hipError_t e = launch_guided_apply(image, depth, n, h, w, dh, dw, c, radius, plan, out, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_guided_depth_apply");
}

int cs_depth_dilate(const float* depth, int n, int h, int w, int c, int radius, int shape, int near, float threshold, float* out,
                    void* stream) {
    const size_t px = (size_t)n * h * w;
    const span buf[2] = {{depth, px * c * 4}, {out, px * 4}};
    if (any_null(buf, 2)) return fail(CS_EINVAL, "null pointer");
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return fail(CS_EINVAL, "non-positive size");
    if (int rc = depth_limits("cs_depth_dilate", n, h, w)) return rc;
    if (radius < 1 || radius > 8) return fail(CS_EINVAL, "cs_depth_dilate: the radius must lie in 1..8");
    if (shape != CS_DILATE_SQUARE && shape != CS_DILATE_DISC) return fail(CS_EINVAL, "cs_depth_dilate: unknown shape");
    if (near != CS_DILATE_NEAR_BRIGHT && near != CS_DILATE_NEAR_DARK) return fail(CS_EINVAL, "cs_depth_dilate: unknown near");
    if (!(threshold >= 0.0f)) return fail(CS_EINVAL, "cs_depth_dilate: threshold must be >= 0 (+inf allowed)");
    if (misaligned(4, buf, 2)) return fail(CS_EINVAL, "cs_depth_dilate: every buffer needs 4-byte alignment");
    if (any_overlap(buf, 2, nullptr, 0)) return fail(CS_EINVAL, "cs_depth_dilate: out must not overlap depth (the halo reads neighbours)");
    hipError_t e = launch_depth_dilate(depth, n, h, w, c, radius, shape, near, threshold, out, (hipStream_t)stream);
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_depth_dilate");
}

int cs_profile(int enable) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof_on.store(enable != 0);
    if (enable) {   // a new measurement: events and tile counts start from zero (switching off keeps them readable)
        g_prof_used = 0;
        g_prof_tiles_any = false; g_prof_tiles_stream = nullptr;
        if (!g_prof_tiles && hipMalloc(&g_prof_tiles, 16) != hipSuccess) { g_prof_tiles = nullptr; (void)hipGetLastError(); }
        if (g_prof_tiles && hipMemset(g_prof_tiles, 0, 16) != hipSuccess) return fail_hip(hipGetLastError(), "cs_profile");
    }
    return CS_OK;
}

int cs_debug_set(int key, int value) {
    if (key < 0 || key >= CS_DEBUG_KEYS) return fail(CS_EINVAL, "cs_debug_set: unknown key");
#ifndef CS_DEV
    if (key == CS_DEBUG_DBG && value != 0 && value != 14 && value != 17 && value != 30 && value != 31)   // (30 / 31: column ranges of the polylines row kernel forced / off: same pixels)
        return fail(CS_EINVAL, "cs_debug_set: this CS_DEBUG_DBG value needs a -DCS_DEV build (phase cut-offs leave outputs unwritten)");
#endif
    if (key == CS_DEBUG_PT_VARIANT) {
        switch (value) {
        case PTV_DEFAULT: case PTV_FIRST_GEN: case PTV_GW_THREADS_512: case PTV_GW_THREADS_256_NARROW: case PTV_GW_THREADS_1024:
        case PTV_GW_SIX_WAVES: case PTV_GW_GENERIC_LAYOUT: case PTV_GW_THREADS_256: case PTV_GW_NO_QUAD: case PTV_LEAN_WHOLE_ROWS:
        case PTV_REPLAY_WAVE_ONLY: case PTV_NAIVE_NO_TIER2: case PTV_TINY_REPLAY_POOL: case PTV_NO_POINT_TIER2: case PTV_SOFT_POINT_TIER2: break;
        default: return fail(CS_EINVAL, "cs_debug_set: unknown CS_DEBUG_PT_VARIANT value (PTV_* in cs_common.h)");
        }
    }
    if (key == CS_DEBUG_ATTN_WAVES && value != 0 && value != 1 && value != 2 && value != 4)
        return fail(CS_EINVAL, "cs_debug_set: CS_DEBUG_ATTN_WAVES takes 0 (the launcher's choice), 1, 2 or 4");
    g_dev[key].store(value, std::memory_order_relaxed);
    return CS_OK;
}

int cs_profile_read(double* total_ms, int* launches) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    double tot = 0.0;
    for (int i = 0; i < g_prof_used; i++) {
        hipError_t e = hipEventSynchronize(g_prof_ev[2 * i + 1]);
        if (e != hipSuccess) return fail_hip(e, "cs_profile_read");
        float ms = 0.0f;
        e = hipEventElapsedTime(&ms, g_prof_ev[2 * i], g_prof_ev[2 * i + 1]);
        if (e != hipSuccess) return fail_hip(e, "cs_profile_read");
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = g_prof_used;
    g_prof_used = 0;
    return CS_OK;
}

// Which share of the 64 x 32 tiles of the cs_generate calls profiled since cs_profile(1) had been written to the blurred depth maps
// (the others are read from the shared gray depth by both eyes: 4 instead of 8 bytes per pixel of depth input for the warp
// kernel), over all their chunks.  Blocking (waits for the last such call's stream, copies two words from a buffer the library
// owns).  *fraction = -1: none of those calls used lazy tiles.
int cs_profile_tiles(double* fraction) {
    if (!fraction) return fail(CS_EINVAL, "null pointer");
    std::lock_guard<std::mutex> lock(g_prof_mu);
    *fraction = -1.0;
    if (!g_prof_tiles || !g_prof_tiles_any) return CS_OK;
    unsigned long long host[2] = {0, 0};
    hipError_t e = hipStreamSynchronize(g_prof_tiles_stream);
    if (e == hipSuccess) e = hipMemcpy(host, g_prof_tiles, 16, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail_hip(e, "cs_profile_tiles");
    if (host[1]) *fraction = (double)host[0] / (double)host[1];
    return CS_OK;
}

int cs_test_powf(const float* x, float y, float* out, size_t count, void* stream) {
    if (!x || !out) return fail(CS_EINVAL, "null pointer");
    hipLaunchKernelGGL(k_test_powf, dim3(grid_for(count, 256)), dim3(256), 0, (hipStream_t)stream, x, y, out, count);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_test_powf");
}

float cs_test_edge_threshold(float den) { return blur_edge_threshold_host(den); }

int cs_test_blur_plan(double blur_strength, double blur_mask_width, int vert_smooth_px, double falloff_exponent, int n, int h, int w,
                      int flags) {
    if (n <= 0 || h <= 0 || w <= 0) return CS_EINVAL;
    const BlurParams prm = {blur_strength, 20.0, blur_mask_width, falloff_exponent, vert_smooth_px};
    return blur_plan_describe(prm, n, h, w, flags);
}

int cs_test_exp(const double* x, double* out, size_t count, void* stream) {
    if (!x || !out) return fail(CS_EINVAL, "null pointer");
    hipLaunchKernelGGL(k_test_exp, dim3(grid_for(count, 256)), dim3(256), 0, (hipStream_t)stream, x, out, count);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? CS_OK : fail_hip(e, "cs_test_exp");
}

}  // extern "C"
