// cs_depthrange.hip -- robust, temporally stable depth range clipping of a video batch (cs_depth_range; DESIGN.md section 5,
// "Depth range clipping").  Not in the reference, which normalises every frame by its own extremes: two order statistics of the
// gray depth per frame, smoothed along t, and a clamp to them, in front of cs_generate.  tools/range_oracle.py states it in numpy.
//
//   g_t      = gray value of frame t (gray_of for C == 3, the value for C == 1, channel 0 otherwise: cs_gray4.h)
//   key(x)   = bits(x) ^ 0x80000000 if the sign bit is clear, else ~bits(x): uint32, monotone in x, -0 below +0
//   raw_lo_t = the element of g_t whose key has rank rank_lo (0-based) among the frame's h * w keys; raw_hi_t: rank_hi
//   lo_t     = raw_lo_t if there is no predecessor, cut[t] != 0 or s is not finite, else s = lo_{t-1} + beta * (raw_lo_t - lo_{t-1})
//   y        = g where g is NaN, else g < lo_t ? lo_t : g, then > hi_t ? hi_t : that (a NaN bound clamps nothing);
//              normalize: hi_t == lo_t ? 0 : (y - lo_t) / (hi_t - lo_t), IEEE division
// float32 throughout, every operation rounded once (-ffp-contract=off).
//
// Exact selection by radix over the key, digits of 11 / 11 / 10 bits from the top, both ranks at once, all frames per launch.
// Seven launches on the caller's stream (one of them a memset), no wait for the device, nothing read back by the host:
//   memset             the workspace's histograms: [n][3 passes][2 ranks][2048] int32, and its selections [n][2][4] int32
//   k_range_hist<P, CM, VEC>   P = 1, 2, 3; grid (ranges, n): workgroup (b, t) owns pixels [b * RH_CHUNK, (b + 1) * RH_CHUNK) of
//                      frame t; lane `tid` owns pixels b * RH_CHUNK + j * 1024 + 4 * tid + {0..3} of trip j (16-byte loads; VEC
//                      false: the same pixels through guarded 4-byte loads).  P == 1 counts every key's top digit into one
//                      histogram (both ranks share it) and, for C != 1, writes g into `out`, where the later passes and the
//                      apply pass read it.  P >= 2 first RESOLVES pass P - 1 (below) -- the pick step, fused into the head of
//                      the launch: every workgroup repeats it for its frame (two 8 KB histograms from L2 against 128 KB of
//                      pixels), workgroup 0 of the frame records it -- then counts, per rank, the keys whose higher digits
//                      equal the rank's prefix.  Where both ranks have one prefix the two histograms would coincide: one is
//                      counted and both ranks are picked from it.
//                      Counts go to int32 bins in LDS (2 x 2048, 16 KB) by ds_add and are then added to the frame's histogram
//                      in global memory by integer atomics, non-zero bins only (integer sums are exact in any order; per-
//                      workgroup partial histograms would cost 16 KB written and read per 128 KB of pixels and a workspace of
//                      n * ranges * 16 KB, the atomics touch the few bins a workgroup filled: the top digit of depth in 0..1
//                      has about a dozen values, and the later passes count only the keys under one prefix).
//                      Bin contention: lanes that hit ONE bin serialise in LDS, and few distinct values per wave is the
//                      ordinary case (every pass-1 histogram of real depth, every 8-bit map, a constant frame).  So a wave
//                      run-length encodes each of its four pixel slots before the add: a lane compares its bin with its left
//                      neighbour's (DPP wave_shr:1), the heads of runs are balloted, and only a head adds, once, its run's
//                      length (the distance to the next head bit).  A constant wave costs one ds_add per slot instead of a
//                      64-deep serial one; noise costs the ballot and the bit scan on top of what it cost anyway.
//   resolve<P>         (device function, the whole workgroup) the pick after pass P: the frame's histogram through an LDS scan
//                      (block_scan_inclusive), the bin whose cumulative count passes the rank, the rank's remainder inside the bin.
//   k_range_pick       one workgroup per frame: resolve<3>; the 32-bit prefix is the key -> raw_lo, raw_hi
//   k_range_smooth     one workgroup: the bounds staged through LDS, the recurrence over t in ONE thread, the state written
//   k_range_apply<VEC> grid (ranges, n): clamp, normalise if asked; reads the input (C == 1) or `out` in place (C != 1)
//
// Bytes per pixel and frame (h * w % 4 == 0):   C == 1: 4 + 4 + 4 read, apply 4 + 4 = 20     C == 3: 12 + 4 written, 4, 4, apply 4 + 4 = 32
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2; no kernel spills a vector or scalar register, none
// uses scratch):                       VGPRs  SGPRs  LDS bytes  occupancy (waves / SIMD)
//   k_range_hist<1, 1, true>             20     28    16384        8
//   k_range_hist<1, 1, false>            24     36    16384        8
//   k_range_hist<1, 3, true>             32     38    16384        8
//   k_range_hist<1, 3, false>            32     48    16384        8
//   k_range_hist<1, 0, false>            34     54    16384        8
//   k_range_hist<2, 1, true>             27     38    16464        8
//   k_range_hist<2, 1, false>            27     41    16464        8
//   k_range_hist<3, 1, true>             33     58    16464        8
//   k_range_hist<3, 1, false>            33     58    16464        8
//   k_range_pick                         33     51    16464        8
//   k_range_smooth                       32     48    12288        8
//   k_range_apply<true>                  16     22        0        8
//   k_range_apply<false>                 22     28        0        8
#include "cs_common.h"
#include "cs_gray4.h"
#include "cs_kernels.h"

namespace cs {

enum { RH_THREADS = 256, RH_TRIPS = 32, RH_TRIP_PX = RH_THREADS * 4, RH_CHUNK = RH_TRIP_PX * RH_TRIPS, RH_BINS = 2048,
       RH_HIST_WORDS = 3 * 2 * RH_BINS, RH_SEL_WORDS = 2 * 4, RS_STAGE = 1024, RA_TRIPS = 4 };

size_t range_chunks(size_t hw) { return (hw + RH_CHUNK - 1) / RH_CHUNK; }
size_t range_workspace_bytes(int n) { return al256((size_t)n * (RH_HIST_WORDS + RH_SEL_WORDS) * 4); }

__device__ __forceinline__ uint32_t key_of(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t key) {
    return __builtin_bit_cast(float, (key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

// One pixel slot of a whole wave into `hist` (LDS): bin < 0 -- the lane's pixel is not counted.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_count(int* hist, int bin, int lane) {
    const int left = __builtin_amdgcn_update_dpp(-2, bin, 0x138 /* wave_shr:1; lane 0 keeps -2 */, 0xf, 0xf, false);
    const bool head = left != bin;
    const unsigned long long heads = __ballot(head);
    if (head && bin >= 0) {
        // the run ends in front of the next head; a bit at 63 - lane stands for the end of the wave
        const unsigned long long rest = ((heads >> lane) >> 1) | (0x8000000000000000ull >> lane);
        atomicAdd(&hist[bin], __builtin_ctzll(rest) + 1);
    }
}

struct Sel { uint32_t prefix[2]; int rank[2]; };   // per rank (lo, hi): the key's digits chosen so far, the rank inside them

// The pick after pass P for frame t, by the whole workgroup: -> the prefixes of P digits and the ranks inside their bins.
// s: 2 x RH_BINS ints of LDS (left dirty), wsum: 16 ints, res: 4 ints.
template <int P>
__device__ Sel resolve(const int32_t* __restrict__ hist, const int32_t* __restrict__ sel, int t, int rank_lo, int rank_hi, int* s,
                       int* wsum, int* res) {
    const int tid = threadIdx.x;
    Sel q;
    q.prefix[0] = q.prefix[1] = 0u;
    q.rank[0] = rank_lo; q.rank[1] = rank_hi;
    if (P > 1) {
        const int32_t* r = sel + ((size_t)t * 2 + (P - 2)) * 4;
        q.prefix[0] = (uint32_t)r[0]; q.rank[0] = r[1]; q.prefix[1] = (uint32_t)r[2]; q.rank[1] = r[3];
    }
    const bool same = q.prefix[0] == q.prefix[1];   // one histogram was counted for both ranks
    const int32_t* H = hist + ((size_t)t * 3 + (P - 1)) * 2 * RH_BINS;
    const int words = same ? RH_BINS : 2 * RH_BINS;
    for (int i = tid; i < words; i += RH_THREADS) s[i] = H[i];
    if (tid < 4) res[tid] = 0;
    __syncthreads();
    block_scan_inclusive(s, RH_BINS, 0, OpAdd(), wsum);
    if (!same) block_scan_inclusive(s + RH_BINS, RH_BINS, 0, OpAdd(), wsum);
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int* a = s + ((r == 1 && !same) ? RH_BINS : 0);
        for (int k = 0; k < RH_BINS / RH_THREADS; k++) {
            const int b = tid * (RH_BINS / RH_THREADS) + k;
            const int below = b > 0 ? a[b - 1] : 0;
            if (below <= q.rank[r] && q.rank[r] < a[b]) { res[2 * r] = b; res[2 * r + 1] = q.rank[r] - below; }
        }
    }
    __syncthreads();
    const int bits = P == 3 ? 10 : 11;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        q.prefix[r] = (q.prefix[r] << bits) | (uint32_t)res[2 * r];
        q.rank[r] = res[2 * r + 1];
    }
    __syncthreads();   // (res and s are written again by the caller)
    return q;
}

template <int P, int CM, bool VEC>
__global__ void __launch_bounds__(RH_THREADS) k_range_hist(const float* __restrict__ src, int c, size_t hw, int rank_lo, int rank_hi,
                                                           float* __restrict__ gray_out, int32_t* __restrict__ hist,
                                                           int32_t* __restrict__ sel) {
    __shared__ int bins[2 * RH_BINS];
    __shared__ int wsum[16];
    __shared__ int res[4];
    const int tid = threadIdx.x, lane = lane_id(), t = blockIdx.y;
    uint32_t plo = 0u, phi = 0u;
    if (P > 1) {
        const Sel q = resolve<P - 1>(hist, sel, t, rank_lo, rank_hi, bins, wsum, res);
        plo = q.prefix[0]; phi = q.prefix[1];
        if (blockIdx.x == 0 && tid == 0) {
            int32_t* r = sel + ((size_t)t * 2 + (P - 2)) * 4;
            r[0] = (int32_t)plo; r[1] = q.rank[0]; r[2] = (int32_t)phi; r[3] = q.rank[1];
        }
    }
    const bool two = P > 1 && plo != phi;
    for (int i = tid; i < 2 * RH_BINS; i += RH_THREADS) bins[i] = 0;
    __syncthreads();
    const float* cur = src + (size_t)t * hw * (CM == 1 ? 1 : c);
    float* gout = (P == 1 && CM != 1) ? gray_out + (size_t)t * hw : nullptr;
    const size_t chunk = (size_t)blockIdx.x * RH_CHUNK;
    constexpr int SHIFT = P == 1 ? 21 : (P == 2 ? 10 : 0);       // the digit's lowest bit
    constexpr uint32_t MASK = P == 3 ? 1023u : 2047u;
#pragma unroll 2
    for (int j = 0; j < RH_TRIPS; j++) {
        if (chunk + (size_t)j * RH_TRIP_PX >= hw) break;          // (uniform over the workgroup: wave_count needs whole waves)
        const size_t i = chunk + (size_t)j * RH_TRIP_PX + 4 * (size_t)tid;
        const bool inside = i < hw;                               // (VEC: h * w is a multiple of 4, so i + 3 < hw as well)
        Px4 g;
        g.v[0] = g.v[1] = g.v[2] = g.v[3] = 0.0f;
        if (inside) g = load_gray4<CM, VEC>(cur, i, hw, c);
        if (P == 1 && CM != 1 && inside) store4<VEC>(gout, i, hw, g);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool live = VEC ? inside : i + k < hw;
            const uint32_t key = key_of(g.v[k]);
            const int digit = (int)((key >> SHIFT) & MASK);
            if (P == 1) {
                wave_count(bins, live ? digit : -1, lane);
            } else {
                const uint32_t high = key >> (SHIFT + (P == 2 ? 11 : 10));
                wave_count(bins, (live && high == plo) ? digit : -1, lane);
                if (two) wave_count(bins + RH_BINS, (live && high == phi) ? digit : -1, lane);   // (uniform branch)
            }
        }
    }
    __syncthreads();
    int32_t* H = hist + ((size_t)t * 3 + (P - 1)) * 2 * RH_BINS;
    const int words = two ? 2 * RH_BINS : RH_BINS;
    for (int i = tid; i < words; i += RH_THREADS) {
        const int v = bins[i];
        if (v != 0) atomicAdd(&H[i], v);
    }
}

__global__ void __launch_bounds__(RH_THREADS) k_range_pick(const int32_t* __restrict__ hist, const int32_t* __restrict__ sel,
                                                           float* __restrict__ raw_lo, float* __restrict__ raw_hi) {
    __shared__ int bins[2 * RH_BINS];
    __shared__ int wsum[16];
    __shared__ int res[4];
    const int t = blockIdx.x;
    const Sel q = resolve<3>(hist, sel, t, 0, 0, bins, wsum, res);
    if (threadIdx.x == 0) {
        raw_lo[t] = value_of(q.prefix[0]);
        raw_hi[t] = value_of(q.prefix[1]);
    }
}

__device__ __forceinline__ float smooth_bound(float prev, float raw, float beta, bool take_raw) {
    const float diff = raw - prev;
    const float s = prev + beta * diff;
    return (take_raw || !(fabsf(s) < INFINITY)) ? raw : s;
}

__global__ void __launch_bounds__(RH_THREADS) k_range_smooth(const float* __restrict__ raw_lo, const float* __restrict__ raw_hi,
                                                             const int32_t* __restrict__ cut, int n, float beta, float* state_lo,
                                                             float* state_hi, int32_t* state_valid, float* __restrict__ lo,
                                                             float* __restrict__ hi) {
    __shared__ float slo[RS_STAGE], shi[RS_STAGE];
    __shared__ int32_t scut[RS_STAGE];
    const int tid = threadIdx.x;
    bool has = false;
    float plo = 0.0f, phi = 0.0f;
    if (tid == 0) { has = state_valid[0] != 0; plo = state_lo[0]; phi = state_hi[0]; }
    for (int t0 = 0; t0 < n; t0 += RS_STAGE) {
        const int len = min((int)RS_STAGE, n - t0);
        for (int i = tid; i < len; i += RH_THREADS) {
            slo[i] = raw_lo[t0 + i]; shi[i] = raw_hi[t0 + i]; scut[i] = cut ? cut[t0 + i] : 0;
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < len; i++) {
                const bool take_raw = !has || scut[i] != 0;
                plo = smooth_bound(plo, slo[i], beta, take_raw);
                phi = smooth_bound(phi, shi[i], beta, take_raw);
                slo[i] = plo; shi[i] = phi;
                has = true;
            }
        }
        __syncthreads();
        for (int i = tid; i < len; i += RH_THREADS) { lo[t0 + i] = slo[i]; hi[t0 + i] = shi[i]; }
        __syncthreads();
    }
    if (tid == 0) { state_lo[0] = plo; state_hi[0] = phi; state_valid[0] = 1; }
}

// src and out are the same array for C != 1 (a lane reads its own pixels before it writes them): no __restrict__
template <bool VEC>
__global__ void __launch_bounds__(RH_THREADS) k_range_apply(const float* src, float* out, size_t hw, const float* __restrict__ lo,
                                                            const float* __restrict__ hi, int normalize) {
    const int t = blockIdx.y;
    const float l = lo[t], h = hi[t];
    const float span = h - l;
    const bool flat = h == l;
    const float* cur = src + (size_t)t * hw;
    float* dst = out + (size_t)t * hw;
#pragma unroll
    for (int j = 0; j < RA_TRIPS; j++) {
        const size_t i = ((size_t)blockIdx.x * RA_TRIPS + j) * RH_TRIP_PX + 4 * (size_t)threadIdx.x;
        if (i >= hw) break;
        Px4 g = load_gray4<1, VEC>(cur, i, hw, 1);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float x = g.v[k];
            float y = x < l ? l : x;
            y = y > h ? h : y;          // (a NaN pixel fails both comparisons and passes; so does every pixel against a NaN bound)
            if (normalize) y = flat ? 0.0f : (y - l) / span;
            g.v[k] = y;
        }
        store4<VEC>(dst, i, hw, g);
    }
}

hipError_t launch_depth_range(const float* depth, int n, int h, int w, int c, int rank_lo, int rank_hi, float beta, int normalize,
                              const int32_t* cut, float* state_lo, float* state_hi, int32_t* state_valid, float* out, float* lo,
                              float* hi, float* raw_lo, float* raw_hi, void* workspace, hipStream_t stream) {
    const size_t hw = (size_t)h * w;
    const bool vec = vec4_path(hw, {depth, out});
    int32_t* hist = (int32_t*)workspace;
    int32_t* sel = hist + (size_t)n * RH_HIST_WORDS;
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)n * (RH_HIST_WORDS + RH_SEL_WORDS) * 4, stream);
    if (e != hipSuccess) return e;
    const dim3 hgrid((unsigned)range_chunks(hw), (unsigned)n), block(RH_THREADS);
#define CS_RANGE_HIST(P, CM, VEC, SRC) \
    hipLaunchKernelGGL((k_range_hist<P, CM, VEC>), hgrid, block, 0, stream, SRC, c, hw, rank_lo, rank_hi, out, hist, sel)
    if (c == 1) { if (vec) CS_RANGE_HIST(1, 1, true, depth); else CS_RANGE_HIST(1, 1, false, depth); }
    else if (c == 3) { if (vec) CS_RANGE_HIST(1, 3, true, depth); else CS_RANGE_HIST(1, 3, false, depth); }
    else CS_RANGE_HIST(1, 0, false, depth);   // (channel 0 of c: strided 4-byte loads on either grid)
    const float* gray = c == 1 ? depth : out;
    if (vec) { CS_RANGE_HIST(2, 1, true, gray); CS_RANGE_HIST(3, 1, true, gray); }
    else { CS_RANGE_HIST(2, 1, false, gray); CS_RANGE_HIST(3, 1, false, gray); }
#undef CS_RANGE_HIST
    hipLaunchKernelGGL(k_range_pick, dim3((unsigned)n), block, 0, stream, (const int32_t*)hist, (const int32_t*)sel, raw_lo, raw_hi);
    hipLaunchKernelGGL(k_range_smooth, dim3(1), block, 0, stream, (const float*)raw_lo, (const float*)raw_hi, cut, n, beta, state_lo,
                       state_hi, state_valid, lo, hi);
    const dim3 agrid((unsigned)((hw + RA_TRIPS * RH_TRIP_PX - 1) / (RA_TRIPS * RH_TRIP_PX)), (unsigned)n);
    if (vec) hipLaunchKernelGGL(k_range_apply<true>, agrid, block, 0, stream, gray, out, hw, (const float*)lo, (const float*)hi, normalize);
    else hipLaunchKernelGGL(k_range_apply<false>, agrid, block, 0, stream, gray, out, hw, (const float*)lo, (const float*)hi, normalize);
    return hipGetLastError();
}

}  // namespace cs
