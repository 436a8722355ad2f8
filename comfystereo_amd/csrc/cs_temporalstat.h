// cs_temporalstat.h -- the scene-cut statistic of the temporal depth filters (cs_temporal.hip, cs_motiondepth.hip):
//   m_t   = mean over the pixels of |g_t - g_{t-1}|          (t == 0: g_{-1} = the state's prev_raw)
//   cut_t = m_t > cut_threshold, or no predecessor
// The two passes must agree bit for bit on m and cut (with search_range 0 the motion-compensated filter IS the plain one), and the
// order of the sum is part of m's value, so the two kernels and their launch live here and nowhere else.  cs_temporal.hip's
// header comment describes them (k_temporal_stat, k_temporal_final), their summation order and their registers.
#pragma once
#include "cs_common.h"
#include "cs_gray4.h"

namespace cs {

enum { TS_THREADS = 256, TS_TRIPS = 16, TS_TRIP_PX = TS_THREADS * 4, TS_CHUNK = TS_TRIP_PX * TS_TRIPS, TF_STAGE = 1024 };

inline size_t temporal_partials(size_t hw) { return (hw + TS_CHUNK - 1) / TS_CHUNK; }

template <int CM, bool VEC>
__global__ void __launch_bounds__(TS_THREADS) k_temporal_stat(const float* __restrict__ depth, int c, size_t hw,
                                                              const float* __restrict__ prev_raw, float* __restrict__ gray_out,
                                                              float* __restrict__ partial, int P) {
    __shared__ float red[TS_THREADS];
    const int tid = threadIdx.x, t = blockIdx.y;
    const float* cur = depth + (size_t)t * hw * c;
    const float* pre = depth + (size_t)(t > 0 ? t - 1 : 0) * hw * c;
    float* gout = (CM != 1) ? gray_out + (size_t)t * hw : nullptr;
    const size_t base = (size_t)blockIdx.x * TS_CHUNK + 4 * (size_t)tid;
    float acc = 0.0f;
#pragma unroll 4
    for (int j = 0; j < TS_TRIPS; j++) {
        const size_t i = base + (size_t)j * TS_TRIP_PX;
        if (i >= hw) break;
        const Px4 g = load_gray4<CM, VEC>(cur, i, hw, c);
        // (uniform over the workgroup: frame 0's predecessor is the state's one-channel gray frame)
        const Px4 p = t > 0 ? load_gray4<CM, VEC>(pre, i, hw, c) : load_gray4<1, VEC>(prev_raw, i, hw, 1);
        if (CM != 1) store4<VEC>(gout, i, hw, g);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (VEC || i + k < hw) acc = acc + fabsf(g.v[k] - p.v[k]);
    }
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int half = TS_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) red[tid] = red[tid] + red[tid + half];
        __syncthreads();
    }
    if (tid == 0) partial[(size_t)t * P + blockIdx.x] = red[0];
}

// (a template so that both files may hold it: THREADS is TS_THREADS)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_temporal_final(const float* __restrict__ partial, int P, float count, float cut_thr,
                                                            const int32_t* __restrict__ valid, float* __restrict__ m,
                                                            int32_t* __restrict__ cut) {
    __shared__ float stage[TF_STAGE];
    const int tid = threadIdx.x, t = blockIdx.x;
    const float* src = partial + (size_t)t * P;
    float s = 0.0f;
    for (int b0 = 0; b0 < P; b0 += TF_STAGE) {
        const int len = min((int)TF_STAGE, P - b0);
        for (int i = tid; i < len; i += THREADS) stage[i] = src[b0 + i];
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < len; i++) s = s + stage[i];
        __syncthreads();
    }
    if (tid == 0) {
        const float mean = s / count;
        const bool has_pred = t > 0 || valid[0] != 0;
        m[t] = has_pred ? mean : 0.0f;
        cut[t] = has_pred ? (mean > cut_thr ? 1 : 0) : 1;   // (a NaN mean is not a cut)
    }
}

// The statistic's two launches: partial [n][P] float32, P = temporal_partials(h * w); gray_out [n][h * w] is written for c != 1;
// vec: vec4_path over depth, gray_out and prev_raw (and whatever else the caller's later kernels take on the same path).
inline void launch_temporal_stat(const float* depth, int n, size_t hw, int c, float cut_thr, const float* prev_raw, const int32_t* valid,
                                 float* gray_out, float* m, int32_t* cut, float* partial, bool vec, hipStream_t stream) {
    const int P = (int)temporal_partials(hw);
    const dim3 sgrid((unsigned)P, (unsigned)n), block(TS_THREADS);
#define CS_TEMPORAL_STAT(CM, VEC) \
    hipLaunchKernelGGL((k_temporal_stat<CM, VEC>), sgrid, block, 0, stream, depth, c, hw, prev_raw, gray_out, partial, P)
    if (c == 1) { if (vec) CS_TEMPORAL_STAT(1, true); else CS_TEMPORAL_STAT(1, false); }
    else if (c == 3) { if (vec) CS_TEMPORAL_STAT(3, true); else CS_TEMPORAL_STAT(3, false); }
    else CS_TEMPORAL_STAT(0, false);   // (channel 0 of c: strided 4-byte loads on either grid)
#undef CS_TEMPORAL_STAT
    hipLaunchKernelGGL(k_temporal_final<TS_THREADS>, dim3((unsigned)n), block, 0, stream, (const float*)partial, P, (float)hw, cut_thr,
                       valid, m, cut);
}

}  // namespace cs
