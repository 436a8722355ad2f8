// cs_nullloss.h -- what the single-tensor kernels of null-text optimisation (cs_inversion.hip: k_null_loss_grad,
// k_null_loss_final, k_adam_step) and their per-frame forms (cs_inversion_frames.hip) share: the reduction's shape, the two-sum
// tree, the per-element body of the loss and the per-element Adam step.  One statement of each, so a frame of the batched
// kernels cannot drift from the single-tensor result the fixtures pin: the same 32 768-element blocks, the same 1024-thread
// strided order inside a block, the same tree, the same second stage.
#pragma once
#include "cs_common.h"
#include "cs_ddimstep.h"

namespace cs {

constexpr int INV_THREADS = 1024;            // the reduction's workgroup
constexpr size_t INV_BLOCK_ELEMS = 32768;    // elements per workgroup of k_null_loss_grad: up to here one launch does it all

inline size_t null_loss_blocks(size_t n) { return (n + INV_BLOCK_ELEMS - 1) / INV_BLOCK_ELEMS; }

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

// One thread's share of block `block` of a tensor of n elements: rec, grad and the thread's pair of the squares' sum.  The
// pointers are the tensor's (a frame's) first element.  PRED: what the model predicts (cs_ddimstep.h).
template <class T, int PRED = CS_PRED_EPSILON>
__device__ __forceinline__ void null_loss_block(const T* __restrict__ eps_uncond, const T* __restrict__ eps_cond,
                                                const T* __restrict__ latent_cur, const T* __restrict__ latent_prev,
                                                T* __restrict__ rec, T* __restrict__ grad, size_t block, size_t n, const StepCoeffs& k,
                                                double grad_scale, float& hi, float& lo) {
    const size_t begin = block * INV_BLOCK_ELEMS;
    const size_t end = begin + INV_BLOCK_ELEMS < n ? begin + INV_BLOCK_ELEMS : n;
    for (size_t i = begin + threadIdx.x; i < end; i += INV_THREADS) {
        const float e = guided<T>((float)eps_uncond[i], (float)eps_cond[i], true, k.guidance);
        rec[i] = (T)ddim_value<T, PRED>((float)latent_cur[i], e, k);
        // loss and gradient: from the reconstruction before its roundings to T (float64 per element, which the bound against a
        // float64 restatement asks for at small counts); each square enters the float32 sum rounded once
        const double a = (double)(float)eps_uncond[i];
        const double e64 = a + (double)k.guidance * ((double)(float)eps_cond[i] - a);
        const double r64 = ddim_value_f64<PRED>((double)(float)latent_cur[i], e64, k);
        const double diff = r64 - (double)(float)latent_prev[i];
        grad[i] = (T)(float)(grad_scale * diff);
        two_sum_add(hi, lo, (float)(diff * diff));
    }
}

// One thread's share of the second stage: the pairs of `blocks` workgroups, strided
__device__ __forceinline__ void null_loss_final_share(const float* __restrict__ partial, int blocks, float& hi, float& lo) {
    for (int b = threadIdx.x; b < blocks; b += INV_THREADS) {
        two_sum_add(hi, lo, partial[2 * b]);
        lo += partial[2 * b + 1];
    }
}

__device__ __forceinline__ float null_loss_mean(float hi, float lo, float count) { return (hi + lo) / count; }

struct AdamCoeffs {
    float w1, beta2, w2, bc2_sqrt, eps, neg_step_size;
};

// torch/optim/adam.py _single_tensor_adam on element i, operation by operation: lerp_, mul_, addcmul_, sqrt, div, add_, addcdiv_
template <class T>
__device__ __forceinline__ void adam_element(T* __restrict__ param, const T* __restrict__ grad, T* __restrict__ exp_avg,
                                             T* __restrict__ exp_avg_sq, size_t i, const AdamCoeffs& k) {
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

}  // namespace cs
