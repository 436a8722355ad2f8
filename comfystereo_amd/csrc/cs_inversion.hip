// cs_inversion.hip -- null-text inversion outside the UNet (reference inversion.py): everything between two UNet calls of
// NullInversion.ddim_loop and NullInversion.null_optimization in one launch each.
//
//   k_ddim_step        classifier-free guidance (:88) and one DDIM step; one formula is prev_step (:57-65) and next_step (:67-75),
//                      the host chooses the two alphas:  out = c4 * ((sample - c1 * e) / c2) + c3 * e
//   k_null_loss_grad   the inner step of null_optimization (:198-201) outside the UNet: the guided prediction, prev_step, the
//                      mean squared error against latent_prev, and its closed-form gradient with respect to eps_uncond
//   k_null_loss_final  the second reduction stage, for tensors of more than one workgroup's share
//   k_adam_step        one torch.optim.Adam step (default betas and eps, no weight decay, no amsgrad) on one flat tensor
//
// Arithmetic: every operation of the reference's tensor expression is one operation here, rounded once to the tensors' dtype
// before the next -- float32: plain IEEE (the library is built with -ffp-contract=off); float16 / bfloat16: the operation in
// float32, then the conversion, which is what torch does with a half tensor and a scalar.  No atomics: the loss is summed in a
// fixed order.  The guided prediction and the DDIM expression themselves are cs_ddimstep.h, shared with cs_standardloop.hip.
#include "cs_common.h"
#include "cs_ddimstep.h"
#include "cs_kernels.h"
#include "cs_latent.h"

namespace cs {

namespace {

constexpr int INV_THREADS = 1024;            // the reduction's workgroup
constexpr size_t INV_BLOCK_ELEMS = 32768;    // elements per workgroup of k_null_loss_grad: up to here one launch does it all

// (hi, lo) += x without losing the rounding error of the sum (Knuth's two-sum; float32 throughout)
__device__ __forceinline__ void two_sum_add(float& hi, float& lo, float x) {
    const float s = hi + x;
    const float bb = s - hi;
    const float err = (hi - (s - bb)) + (x - bb);
    hi = s;
    lo += err;
}

// the workgroup's pairs -> thread 0's pair, a fixed tree
__device__ __forceinline__ void block_reduce_pairs(float& hi, float& lo, float* sh_hi, float* sh_lo) {
    const int tid = threadIdx.x;
    sh_hi[tid] = hi;
    sh_lo[tid] = lo;
    __syncthreads();
    for (int half = INV_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) {
            float h = sh_hi[tid], l = sh_lo[tid];
            two_sum_add(h, l, sh_hi[tid + half]);
            l += sh_lo[tid + half];
            sh_hi[tid] = h;
            sh_lo[tid] = l;
        }
        __syncthreads();
    }
    hi = sh_hi[0];
    lo = sh_lo[0];
}

}  // namespace

template <class T>
__global__ void __launch_bounds__(256) k_ddim_step(const T* sample, const T* __restrict__ eps_a, const T* __restrict__ eps_b, T* out,
                                                   size_t n, StepCoeffs k) {
    // out may be sample (neither is __restrict__): every element is read before it is written, by the same thread
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += step) {
        const float e = guided<T>((float)eps_a[i], eps_b ? (float)eps_b[i] : 0.0f, eps_b != nullptr, k.guidance);
        out[i] = (T)ddim_value<T>((float)sample[i], e, k);
    }
}

// grid: blocks of INV_BLOCK_ELEMS consecutive elements.  One block: it writes the loss.  More: partial[2 * block] = its pair.
template <class T>
__global__ void __launch_bounds__(INV_THREADS) k_null_loss_grad(const T* __restrict__ eps_uncond, const T* __restrict__ eps_cond,
                                                                const T* __restrict__ latent_cur, const T* __restrict__ latent_prev,
                                                                T* __restrict__ rec, T* __restrict__ grad, float* __restrict__ loss,
                                                                float* __restrict__ partial, size_t n, StepCoeffs k, double grad_scale,
                                                                float count) {
    __shared__ float sh_hi[INV_THREADS], sh_lo[INV_THREADS];
    const size_t begin = (size_t)blockIdx.x * INV_BLOCK_ELEMS;
    const size_t end = begin + INV_BLOCK_ELEMS < n ? begin + INV_BLOCK_ELEMS : n;
    float hi = 0.0f, lo = 0.0f;
    for (size_t i = begin + threadIdx.x; i < end; i += INV_THREADS) {
        const float e = guided<T>((float)eps_uncond[i], (float)eps_cond[i], true, k.guidance);
        rec[i] = (T)ddim_value<T>((float)latent_cur[i], e, k);
        // loss and gradient: from the reconstruction before its roundings to T (float64 per element, which the bound against a
        // float64 restatement asks for at small counts); each square enters the float32 sum rounded once
        const double a = (double)(float)eps_uncond[i];
        const double e64 = a + (double)k.guidance * ((double)(float)eps_cond[i] - a);
        const double r64 = (double)k.c4 * (((double)(float)latent_cur[i] - (double)k.c1 * e64) / (double)k.c2) + (double)k.c3 * e64;
        const double diff = r64 - (double)(float)latent_prev[i];
        grad[i] = (T)(float)(grad_scale * diff);
        two_sum_add(hi, lo, (float)(diff * diff));
    }
    block_reduce_pairs(hi, lo, sh_hi, sh_lo);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            loss[0] = (hi + lo) / count;
        } else {
            partial[2 * blockIdx.x] = hi;
            partial[2 * blockIdx.x + 1] = lo;
        }
    }
}

__global__ void __launch_bounds__(INV_THREADS) k_null_loss_final(const float* __restrict__ partial, int blocks, float* __restrict__ loss,
                                                                 float count) {
    __shared__ float sh_hi[INV_THREADS], sh_lo[INV_THREADS];
    float hi = 0.0f, lo = 0.0f;
    for (int b = threadIdx.x; b < blocks; b += INV_THREADS) {
        two_sum_add(hi, lo, partial[2 * b]);
        lo += partial[2 * b + 1];
    }
    block_reduce_pairs(hi, lo, sh_hi, sh_lo);
    if (threadIdx.x == 0) loss[0] = (hi + lo) / count;
}

struct AdamCoeffs {
    float w1, beta2, w2, bc2_sqrt, eps, neg_step_size;
};

// torch/optim/adam.py _single_tensor_adam, operation by operation: lerp_, mul_, addcmul_, sqrt, div, add_, addcdiv_
template <class T>
__global__ void __launch_bounds__(256) k_adam_step(T* __restrict__ param, const T* __restrict__ grad, T* __restrict__ exp_avg,
                                                   T* __restrict__ exp_avg_sq, size_t n, AdamCoeffs k) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += step) {
        const float g = (float)grad[i];
        float m = (float)exp_avg[i], v = (float)exp_avg_sq[i];
        // lerp(m, g, w1): torch's two forms around w = 0.5
        m = k.w1 < 0.5f ? rnd<T>(m + k.w1 * (g - m)) : rnd<T>(g - (g - m) * (1.0f - k.w1));
        v = rnd<T>(v * k.beta2);
        v = rnd<T>(v + k.w2 * g * g);
        const float denom = rnd<T>(rnd<T>(rnd<T>(sqrtf(v)) / k.bc2_sqrt) + k.eps);
        const float p = rnd<T>((float)param[i] + k.neg_step_size * m / denom);
        exp_avg[i] = (T)m;
        exp_avg_sq[i] = (T)v;
        param[i] = (T)p;
    }
}

static StepCoeffs step_coeffs(float guidance, const float c[4]) { return StepCoeffs{guidance, c[0], c[1], c[2], c[3]}; }

hipError_t launch_ddim_step(const void* sample, const void* eps_a, const void* eps_b, void* out, int dtype, size_t n, float guidance,
                            const float c[4], hipStream_t stream) {
    const StepCoeffs k = step_coeffs(guidance, c);
    with_latent_type(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(k_ddim_step<T>, dim3(stream_grid(n)), dim3(256), 0, stream, as<T>(sample), as<T>(eps_a), as<T>(eps_b), as<T>(out),
                           n, k);
    });
    return hipGetLastError();
}

static size_t null_loss_blocks(size_t n) { return (n + INV_BLOCK_ELEMS - 1) / INV_BLOCK_ELEMS; }

size_t null_loss_max_count() { return INV_BLOCK_ELEMS * (size_t)0x7fffffff; }   // a 32-bit grid of workgroups

size_t null_loss_workspace_bytes(size_t n) {
    const size_t blocks = null_loss_blocks(n);
    return blocks > 1 ? blocks * 2 * sizeof(float) : 0;
}

hipError_t launch_null_loss_grad(const void* eps_uncond, const void* eps_cond, const void* latent_cur, const void* latent_prev,
                                 void* rec, float* loss, void* grad, int dtype, size_t n, float guidance, const float c[4],
                                 double grad_scale, void* workspace, hipStream_t stream) {
    const int blocks = (int)null_loss_blocks(n);
    const dim3 grid(blocks), block(INV_THREADS);
    const StepCoeffs k = step_coeffs(guidance, c);
    float* partial = (float*)workspace;
    const float count = (float)n;
    with_latent_type(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(k_null_loss_grad<T>, grid, block, 0, stream, as<T>(eps_uncond), as<T>(eps_cond), as<T>(latent_cur),
                           as<T>(latent_prev), as<T>(rec), as<T>(grad), loss, partial, n, k, grad_scale, count);
    });
    if (blocks > 1) hipLaunchKernelGGL(k_null_loss_final, dim3(1), block, 0, stream, partial, blocks, loss, count);
    return hipGetLastError();
}

hipError_t launch_adam_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int dtype, size_t n, const float k6[6],
                            hipStream_t stream) {
    const AdamCoeffs k{k6[0], k6[1], k6[2], k6[3], k6[4], k6[5]};
    with_latent_type(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(k_adam_step<T>, dim3(stream_grid(n)), dim3(256), 0, stream, as<T>(param), as<T>(grad), as<T>(exp_avg),
                           as<T>(exp_avg_sq), n, k);
    });
    return hipGetLastError();
}

}  // namespace cs
