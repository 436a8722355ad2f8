// cs_gaussblur.hip -- the reference's Gaussian depth blurs (stereoimage_generation.py): blur_depth_map (:1253-1281),
// edge_selective_blur_depth_map (:1283-1309), left_direction_aware_blur_depth_map (:1311-1327) and
// right_direction_aware_blur_depth_map (:1329-1344).
//
// Two passes over [n][h][w] float32, np.convolve(np.pad(line, radius, 'edge'), taps, 'valid') along the rows, then along the
// columns of the float32 intermediate (caller's workspace).  Every output is sum_j padded[i + j] * taps[n_taps - 1 - j] for
// ascending j: float32 sample times float64 tap, one float64 multiply and one float64 add per tap (-ffp-contract=off), from
// +0.0, rounded to float32 when stored.  The taps are the caller's float64 array; they are
// uniform over a wave and read through the scalar cache (s_load), never by a per-lane load.
//   k_gauss_rows      one workgroup per GR_TILE columns of a row: the segment and its halo (clamped columns) in LDS; a
//                     thread owns 4 consecutive outputs and slides an 8-sample window over the segment, one ds_read_b128
//                     per 4 taps and 16 multiply-adds; results leave through LDS as whole coalesced rows
//   k_gauss_cols<OP>  one wave per 64 consecutive columns x GC_ROWS output rows (lanes on consecutive columns: every global
//                     access is one coalesced row piece); each loaded row feeds all GC_ROWS accumulators of the band, so a
//                     band reads GC_ROWS + 2 * radius rows, not GC_ROWS * (2 * radius + 1).  The epilogue computes the blend
//                     weight of OP from the 3x3 / 3x1 neighbourhood of the SOURCE depth (clamped indices) and writes
//                     (1 - w) * depth + w * blurred: the blending functions cost no extra pass.
#include "cs_common.h"
#include "cs_kernels.h"

namespace cs {

enum { GR_TILE = 1024, GR_THREADS = 256, GC_ROWS = 16, GC_THREADS = 256, GAUSS_MAX_TAPS = 4097 };   // radius <= 2048

int gaussblur_max_taps() { return GAUSS_MAX_TAPS; }

__host__ __device__ inline size_t gauss_rows_lds_bytes(int n_taps) { return align16((size_t)(GR_TILE + n_taps + 4) * 4); }

__global__ void __launch_bounds__(GR_THREADS) k_gauss_rows(const float* __restrict__ src, const double* __restrict__ taps, int n_taps,
                                                           int w, int ntiles, float* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* seg = (float*)smem;
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % ntiles;
    const size_t row = blockIdx.x / ntiles;
    const int xs = tile * GR_TILE, r = n_taps >> 1;
    const int len = min(GR_TILE, w - xs);
    const float* in = src + row * (size_t)w;
    // seg[i] = padded[xs + i] = row[clamp(xs + i - radius)] for every index a window can touch
    const int span = (((len + 3) & ~3) + n_taps + 3) & ~3;
    for (int i = tid; i < span; i += GR_THREADS) seg[i] = in[min(max(xs + i - r, 0), w - 1)];
    __syncthreads();

    const int x0 = 4 * tid;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (x0 < len) {
        const double* tp = taps + (n_taps - 1);   // tp[-j]: tap j of the flipped array
        int k = 0;
        float4 cur = *reinterpret_cast<const float4*>(seg + x0);
        for (; k + 4 <= n_taps; k += 4) {
            const float4 nxt = *reinterpret_cast<const float4*>(seg + x0 + k + 4);
            const double t0 = tp[-k], t1 = tp[-k - 1], t2 = tp[-k - 2], t3 = tp[-k - 3];
            const double w0 = cur.x, w1 = cur.y, w2 = cur.z, w3 = cur.w, w4 = nxt.x, w5 = nxt.y, w6 = nxt.z;
            a0 = a0 + w0 * t0; a1 = a1 + w1 * t0; a2 = a2 + w2 * t0; a3 = a3 + w3 * t0;
            a0 = a0 + w1 * t1; a1 = a1 + w2 * t1; a2 = a2 + w3 * t1; a3 = a3 + w4 * t1;
            a0 = a0 + w2 * t2; a1 = a1 + w3 * t2; a2 = a2 + w4 * t2; a3 = a3 + w5 * t2;
            a0 = a0 + w3 * t3; a1 = a1 + w4 * t3; a2 = a2 + w5 * t3; a3 = a3 + w6 * t3;
            cur = nxt;
        }
        for (; k < n_taps; k++) {
            const double t = tp[-k];
            const float* s = seg + x0 + k;
            a0 = a0 + (double)s[0] * t; a1 = a1 + (double)s[1] * t; a2 = a2 + (double)s[2] * t; a3 = a3 + (double)s[3] * t;
        }
    }
    __syncthreads();
    if (x0 < len) *reinterpret_cast<float4*>(seg + x0) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
    __syncthreads();
    float* out = dst + row * (size_t)w + xs;
    for (int i = tid; i < len; i += GR_THREADS) out[i] = seg[i];
}

// np.minimum(q, 1): q when q < 1 or q is a NaN
__device__ __forceinline__ float np_min1(float q) { return (q < 1.0f || q != q) ? q : 1.0f; }

// the blend weight of OP at (y, x) of frame plane `d`
template <int OP>
__device__ __forceinline__ float gauss_weight(const float* d, int y, int x, int h, int w, float thr) {
    const int xl = max(x - 1, 0), xr = min(x + 1, w - 1);
    if (OP == CS_GAUSS_EDGE_SELECTIVE) {
        const float* r0 = d + (size_t)max(y - 1, 0) * w;
        const float* r1 = d + (size_t)y * w;
        const float* r2 = d + (size_t)min(y + 1, h - 1) * w;
        const double p[9] = {r0[xl], r0[x], r0[xr], r1[xl], r1[x], r1[xr], r2[xl], r2[x], r2[xr]};
        const double kx[9] = {-1, 0, 1, -2, 0, 2, -1, 0, 1}, ky[9] = {-1, -2, -1, 0, 0, 0, 1, 2, 1};
        double qx[9], qy[9];
#pragma unroll
        for (int i = 0; i < 9; i++) { qx[i] = p[i] * kx[i]; qy[i] = p[i] * ky[i]; }
        // np.sum over nine float64 values: eight pairwise, then the ninth
        const float gx = (float)((((qx[0] + qx[1]) + (qx[2] + qx[3])) + ((qx[4] + qx[5]) + (qx[6] + qx[7]))) + qx[8]);
        const float gy = (float)((((qy[0] + qy[1]) + (qy[2] + qy[3])) + ((qy[4] + qy[5]) + (qy[6] + qy[7]))) + qy[8]);
        return np_min1(sqrtf(gx * gx + gy * gy) / thr);
    }
    const float* r1 = d + (size_t)y * w;
    const float grad = (r1[xr] - r1[xl]) / 2.0f;
    if (OP == CS_GAUSS_LEFT) return grad > 0.0f ? np_min1(grad / thr) : 0.0f;
    return grad < 0.0f ? np_min1(fabsf(grad) / thr) : 0.0f;
}

template <int OP>
__global__ void __launch_bounds__(GC_THREADS) k_gauss_cols(const float* __restrict__ tmp, const float* __restrict__ depth,
                                                           const double* __restrict__ taps, int n_taps, float thr, int h, int w,
                                                           int nct, int nbands, float* __restrict__ out) {
    const int ct = blockIdx.x % nct;
    const int band = (blockIdx.x / nct) % nbands;
    const size_t f = blockIdx.x / ((size_t)nct * nbands);
    const int x = ct * GC_THREADS + threadIdx.x;
    const int xc = min(x, w - 1);           // lanes beyond the row compute a copy of the last column and store nothing
    const int i0 = band * GC_ROWS, r = n_taps >> 1;
    const float* plane = tmp + f * (size_t)h * w;
    const double* tp = taps + (n_taps - 1);   // tp[-j]: tap j of the flipped array
    double acc[GC_ROWS];
#pragma unroll
    for (int q = 0; q < GC_ROWS; q++) acc[q] = 0.0;
    auto sample = [&](int p) { return (double)plane[(size_t)min(max(i0 + p - r, 0), h - 1) * w + xc]; };
    // padded row p of the band (source row clamp(i0 + p - radius)) is tap p - q of output row i0 + q
    auto guarded = [&](int p) {
        const double v = sample(p);
#pragma unroll
        for (int q = 0; q < GC_ROWS; q++) {
            const int t = p - q;
            if (t >= 0 && t < n_taps) acc[q] = acc[q] + v * tp[-t];
        }
    };
    const int total = GC_ROWS - 1 + n_taps;
    const int head = min(GC_ROWS - 1, total), steady_end = max(n_taps, head);
    int p = 0;
    for (; p < head; p++) guarded(p);
#pragma unroll 2
    for (; p < n_taps; p++) {   // every output row of the band has a tap on this row
        const double v = sample(p);
#pragma unroll
        for (int q = 0; q < GC_ROWS; q++) acc[q] = acc[q] + v * tp[q - p];
    }
    for (p = steady_end; p < total; p++) guarded(p);

    if (x >= w) return;
    const float* dpl = depth + f * (size_t)h * w;
    float* opl = out + f * (size_t)h * w;
#pragma unroll
    for (int q = 0; q < GC_ROWS; q++) {
        const int y = i0 + q;
        if (y >= h) break;
        const float blurred = (float)acc[q];
        if (OP == CS_GAUSS_PLAIN) {
            opl[(size_t)y * w + x] = blurred;
        } else {
            const float wt = gauss_weight<OP>(dpl, y, x, h, w, thr);
            const float d = dpl[(size_t)y * w + x];
            opl[(size_t)y * w + x] = (1.0f - wt) * d + wt * blurred;
        }
    }
}

hipError_t launch_gaussblur(int op, const float* depth, const double* taps, int n_taps, double edge_threshold, int n, int h, int w,
                            float* out, float* tmp, hipStream_t stream) {
    const int ntiles = (w + GR_TILE - 1) / GR_TILE;
    const size_t lds = gauss_rows_lds_bytes(n_taps);
    hipLaunchKernelGGL(k_gauss_rows, dim3((unsigned)((size_t)n * h * ntiles)), dim3(GR_THREADS), lds, stream, depth, taps, n_taps, w,
                       ntiles, tmp);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int nct = (w + GC_THREADS - 1) / GC_THREADS, nbands = (h + GC_ROWS - 1) / GC_ROWS;
    const dim3 grid((unsigned)((size_t)n * nct * nbands)), block(GC_THREADS);
    const float thr = (float)edge_threshold;
    switch (op) {
    case CS_GAUSS_PLAIN: hipLaunchKernelGGL(k_gauss_cols<CS_GAUSS_PLAIN>, grid, block, 0, stream, tmp, depth, taps, n_taps, thr, h, w, nct, nbands, out); break;
    case CS_GAUSS_EDGE_SELECTIVE: hipLaunchKernelGGL(k_gauss_cols<CS_GAUSS_EDGE_SELECTIVE>, grid, block, 0, stream, tmp, depth, taps, n_taps, thr, h, w, nct, nbands, out); break;
    case CS_GAUSS_LEFT: hipLaunchKernelGGL(k_gauss_cols<CS_GAUSS_LEFT>, grid, block, 0, stream, tmp, depth, taps, n_taps, thr, h, w, nct, nbands, out); break;
    default: hipLaunchKernelGGL(k_gauss_cols<CS_GAUSS_RIGHT>, grid, block, 0, stream, tmp, depth, taps, n_taps, thr, h, w, nct, nbands, out); break;
    }
    return hipGetLastError();
}

}  // namespace cs
