// cs_inversion.hip -- null-text inversion outside the UNet (reference inversion.py): everything between two UNet calls of
// NullInversion.ddim_loop and NullInversion.null_optimization in one launch each.
//
//   k_ddim_step        classifier-free guidance (:88) and one DDIM step; one formula is prev_step (:57-65) and next_step (:67-75),
//                      the host chooses the two alphas:  out = c4 * ((sample - c1 * e) / c2) + c3 * e; for a v-prediction model
//                      (PRED = CS_PRED_V) the step of cs_ddimstep.h on v
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
#include "cs_nullloss.h"

namespace cs {

template <class T, int PRED>
__global__ void __launch_bounds__(256) k_ddim_step(const T* sample, const T* __restrict__ eps_a, const T* __restrict__ eps_b, T* out,
                                                   size_t n, StepCoeffs k) {
    // out may be sample (neither is __restrict__): every element is read before it is written, by the same thread
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += step) {
        const float e = guided<T>((float)eps_a[i], eps_b ? (float)eps_b[i] : 0.0f, eps_b != nullptr, k.guidance);
        out[i] = (T)ddim_value<T, PRED>((float)sample[i], e, k);
    }
}

// grid: blocks of INV_BLOCK_ELEMS consecutive elements.  One block: it writes the loss.  More: partial[2 * block] = its pair.
template <class T, int PRED>
__global__ void __launch_bounds__(INV_THREADS) k_null_loss_grad(const T* __restrict__ eps_uncond, const T* __restrict__ eps_cond,
                                                                const T* __restrict__ latent_cur, const T* __restrict__ latent_prev,
                                                                T* __restrict__ rec, T* __restrict__ grad, float* __restrict__ loss,
                                                                float* __restrict__ partial, size_t n, StepCoeffs k, double grad_scale,
                                                                float count) {
    __shared__ float sh_hi[INV_THREADS], sh_lo[INV_THREADS];
    float hi = 0.0f, lo = 0.0f;
    null_loss_block<T, PRED>(eps_uncond, eps_cond, latent_cur, latent_prev, rec, grad, blockIdx.x, n, k, grad_scale, hi, lo);
    block_reduce_pairs(hi, lo, sh_hi, sh_lo);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            loss[0] = null_loss_mean(hi, lo, count);
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
    null_loss_final_share(partial, blocks, hi, lo);
    block_reduce_pairs(hi, lo, sh_hi, sh_lo);
    if (threadIdx.x == 0) loss[0] = null_loss_mean(hi, lo, count);
}

template <class T>
__global__ void __launch_bounds__(256) k_adam_step(T* __restrict__ param, const T* __restrict__ grad, T* __restrict__ exp_avg,
                                                   T* __restrict__ exp_avg_sq, size_t n, AdamCoeffs k) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += step) {
        adam_element<T>(param, grad, exp_avg, exp_avg_sq, i, k);
    }
}

static StepCoeffs step_coeffs(float guidance, const float c[4]) { return StepCoeffs{guidance, c[0], c[1], c[2], c[3]}; }

hipError_t launch_ddim_step(const void* sample, const void* eps_a, const void* eps_b, void* out, int dtype, size_t n, float guidance,
                            const float c[4], int prediction, hipStream_t stream) {
    const StepCoeffs k = step_coeffs(guidance, c);
    with_latent_type(dtype, [&](auto tag) {
        using T = decltype(tag);
        with_prediction(prediction, [&](auto pred) {
            hipLaunchKernelGGL((k_ddim_step<T, decltype(pred)::value>), dim3(stream_grid(n)), dim3(256), 0, stream, as<T>(sample),
                               as<T>(eps_a), as<T>(eps_b), as<T>(out), n, k);
        });
    });
    return hipGetLastError();
}

size_t null_loss_max_count() { return INV_BLOCK_ELEMS * (size_t)0x7fffffff; }   // a 32-bit grid of workgroups

size_t null_loss_workspace_bytes(size_t n) {
    const size_t blocks = null_loss_blocks(n);
    return blocks > 1 ? blocks * 2 * sizeof(float) : 0;
}

hipError_t launch_null_loss_grad(const void* eps_uncond, const void* eps_cond, const void* latent_cur, const void* latent_prev,
                                 void* rec, float* loss, void* grad, int dtype, size_t n, float guidance, const float c[4],
                                 int prediction, double grad_scale, void* workspace, hipStream_t stream) {
    const int blocks = (int)null_loss_blocks(n);
    const dim3 grid(blocks), block(INV_THREADS);
    const StepCoeffs k = step_coeffs(guidance, c);
    float* partial = (float*)workspace;
    const float count = (float)n;
    with_latent_type(dtype, [&](auto tag) {
        using T = decltype(tag);
        with_prediction(prediction, [&](auto pred) {
            hipLaunchKernelGGL((k_null_loss_grad<T, decltype(pred)::value>), grid, block, 0, stream, as<T>(eps_uncond), as<T>(eps_cond),
                               as<T>(latent_cur), as<T>(latent_prev), as<T>(rec), as<T>(grad), loss, partial, n, k, grad_scale, count);
        });
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
