// cs_temporal.hip -- temporal depth stabilisation of a video batch (cs_temporal_depth; DESIGN.md section 5, "Temporal depth
// stabilisation").  Not in the reference, which treats every frame alone: a causal, motion-adaptive, scene-cut-aware filter
// along t over the gray depth, with its state carried from call to call.  tools/temporal_oracle.py states it in numpy.
//
//   g_t   = gray value of frame t (gray_of for C == 3, the value for C == 1, channel 0 otherwise: cs_gray4.h, Px4 / load_gray4 / store4)
//   m_t   = mean over the pixels of |g_t - g_{t-1}|          (t == 0: g_{-1} = the state's prev_raw)
//   cut_t = m_t > cut_threshold, or no predecessor
//   y_t   = g_t  if cut_t or !(|g_t - y_{t-1}| < motion_threshold),  else  y_{t-1} + alpha * (g_t - y_{t-1})
// float32 throughout, every operation rounded once (-ffp-contract=off).
//
// Three launches on the caller's stream, no wait for the device, no atomics:
//   k_temporal_stat<CM, VEC>   grid (P, n): workgroup (b, t) owns pixels [b * TS_CHUNK, (b + 1) * TS_CHUNK) of frame t.  Lane `tid`
//                      owns pixels b * TS_CHUNK + j * 1024 + 4 * tid + {0..3} for the trips j = 0 .. TS_TRIPS - 1 and adds their
//                      |g_t - g_{t-1}| to its float32 sum in that order (a serial run of 4 * TS_TRIPS = 64 additions); the 256
//                      sums meet in a fixed pairwise LDS tree (depth 8); partial[t][b] gets the result.  For C != 1 it also writes
//                      g_t into `out`.  The predecessor's gray value is recomputed from frame t - 1 of the input.
//   k_temporal_final   one workgroup per frame: the frame's P partials staged through LDS and added by ONE thread in index order,
//                      divided by (float)(h * w), compared with the threshold -> m, cut.  Frame 0 of a call without valid state:
//                      m = 0, cut = 1.
//   k_temporal_recur<VEC>      one lane per four consecutive pixels, a loop over t in the lane: frames t + 1 and t + 2 are
//                      in flight during frame t's arithmetic (each lane's chain is serial in t: without its own loads in flight a
//                      lane would pay the memory latency n times).  Three fixed register buffers and a loop unrolled by three, so
//                      that no copy out of a load's destination forces a wait: in the 16-byte instantiation every wait inside the
//                      loop leaves the two younger requests outstanding (vmcnt(2); vmcnt(3) before a buffer is requested again),
//                      the one full wait stands in front of the loop.  cut[t] is uniform and read through the scalar cache.  Reads g
//                      from the input (C == 1) or in place from `out` (C != 1); writes y, and after the last frame the state
//                      (prev_raw = g, prev = y of the last frame) and the validity flag.
// The order of every sum depends on h * w alone, not on n, the frame's position in the call or the path: the scalar path (VEC
// false: h * w no multiple of 4, or a buffer off the 16-byte grid) gives a lane the same four pixels through guarded 4-byte
// accesses, so m of a frame pair is the same inside one call, across two calls, and on either path.
//
// Bytes per pixel and frame (h * w % 4 == 0):
//   C == 1   stat 4 + 4 (frame t - 1 again; 33 MB behind at 4K, so from the Infinity Cache)   recurrence 4 + 4    = 16, 12 from HBM
//   C == 3   stat 12 + 12 (likewise) + 4 written                                               recurrence 4 + 4    = 36, 24 from HBM
//   C == 3 WITHOUT the gray map in `out`: stat 12 + 12, recurrence 12 + 4                                          = 40, 28 from HBM
// so the statistic pass writes g into `out` for C != 1 (4 bytes per pixel less, and the recurrence has one instantiation).
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2; no kernel spills a vector or scalar register, none
// uses scratch):                       VGPRs  SGPRs  LDS bytes  occupancy (waves / SIMD)
//   k_temporal_stat<1, true>             20     46     1024        8
//   k_temporal_stat<1, false>            24     80     1024        8
//   k_temporal_stat<3, true>             38     68     1024        8
//   k_temporal_stat<3, false>            32     84     1024        8
//   k_temporal_stat<0, false>            70     88     1024        7
//   k_temporal_final                     14     31     4096        8
//   k_temporal_recur<true>               40     43        0        8
//   k_temporal_recur<false>              27     51        0        8
#include "cs_common.h"
#include "cs_gray4.h"
#include "cs_kernels.h"
#include "cs_temporalstat.h"

// (k_temporal_stat and k_temporal_final: cs_temporalstat.h, shared with cs_motiondepth.hip)
namespace cs {

// src and out are the same array for C != 1 (a lane reads frame t + 2 of its own pixels before it writes frame t): no __restrict__
template <bool VEC>
__global__ void __launch_bounds__(TS_THREADS) k_temporal_recur(const float* src, float* out, int n, size_t hw,
                                                               const int32_t* __restrict__ cut, float alpha, float motion_thr,
                                                               float* prev_raw, float* prev, int32_t* valid) {
    const size_t i = ((size_t)blockIdx.x * TS_THREADS + threadIdx.x) * 4;
    if (blockIdx.x == 0 && threadIdx.x == 0) valid[0] = 1;   // (nothing in this kernel reads it)
    if (i >= hw) return;
    // Three fixed buffers, the loop over t unrolled by three: frame t is worked on in the buffer it was loaded into while the
    // loads of t + 1 and t + 2 are in flight, and frame t + 3 is requested into frame t's buffer once frame t is stored.  (A
    // rotation g0 = g1, g1 = g2 copies out of a load's destination registers and so waits for the newest load every frame.)
    auto frame = [&](int t) { return load_gray4<1, VEC>(src + (size_t)t * hw, i, hw, 1); };
    auto step = [&](int t, const Px4& g, Px4& y) {
        const bool is_cut = cut[t] != 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float delta = g.v[k] - y.v[k];
            const float blend = y.v[k] + alpha * delta;
            y.v[k] = (is_cut || !(fabsf(delta) < motion_thr)) ? g.v[k] : blend;
        }
        store4<VEC>(out + (size_t)t * hw, i, hw, y);
    };
    Px4 y = load_gray4<1, VEC>(prev, i, hw, 1);
    Px4 a = frame(0);
    Px4 b = frame(n > 1 ? 1 : 0);
    Px4 c = frame(n > 2 ? 2 : 0);
    int t = 0;
    for (; t + 3 <= n; t += 3) {
        step(t, a, y);
        if (t + 3 < n) a = frame(t + 3);
        step(t + 1, b, y);
        if (t + 4 < n) b = frame(t + 4);
        step(t + 2, c, y);
        if (t + 5 < n) c = frame(t + 5);
    }
    // one or two frames left in a, b; the last frame's g: n % 3 == 0 -> c (the loop did not reload it), 1 -> a, 2 -> b
    const int left = n - t;
    if (left >= 1) step(t, a, y);
    if (left == 2) step(t + 1, b, y);
    const Px4 g = left == 0 ? c : (left == 1 ? a : b);
    store4<VEC>(prev_raw, i, hw, g);
    store4<VEC>(prev, i, hw, y);
}

size_t temporal_workspace_bytes(int n, int h, int w) { return al256((size_t)n * temporal_partials((size_t)h * w) * 4); }

hipError_t launch_temporal(const float* depth, int n, int h, int w, int c, float alpha, float motion_thr, float cut_thr,
                           float* prev_raw, float* prev, int32_t* valid, float* out, float* m, int32_t* cut, float* partial,
                           hipStream_t stream) {
    const size_t hw = (size_t)h * w;
    const bool vec = vec4_path(hw, {depth, out, prev_raw, prev});
    const dim3 block(TS_THREADS);
    launch_temporal_stat(depth, n, hw, c, cut_thr, prev_raw, valid, out, m, cut, partial, vec, stream);
    const float* src = c == 1 ? depth : out;
    const dim3 rgrid((unsigned)((hw + TS_TRIP_PX - 1) / TS_TRIP_PX));
    if (vec) hipLaunchKernelGGL(k_temporal_recur<true>, rgrid, block, 0, stream, src, out, n, hw, (const int32_t*)cut, alpha, motion_thr, prev_raw, prev, valid);
    else hipLaunchKernelGGL(k_temporal_recur<false>, rgrid, block, 0, stream, src, out, n, hw, (const int32_t*)cut, alpha, motion_thr, prev_raw, prev, valid);
    return hipGetLastError();
}

}  // namespace cs
