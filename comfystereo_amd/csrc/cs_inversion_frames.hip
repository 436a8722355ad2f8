// cs_inversion_frames.hip -- null-text optimisation outside the UNet on F frames at once (cs_null_loss_grad_frames,
// cs_adam_step_frames): the kernels of cs_inversion.hip with a frame axis, for a UNet that runs F frames in one batch while
// every frame keeps its own loss, its own early stop and its own Adam state.
//
//   k_null_loss_grad_frames   grid (blocks per frame, F): workgroup (b, f) is workgroup b of k_null_loss_grad on frame f's `per`
//                             elements alone -- the same blocks counted from the frame's first element, the same strided order,
//                             the same tree (cs_nullloss.h) -- so each frame's rec, grad and loss are the single-tensor bits
//   k_null_loss_final_frames  grid F: the second stage of each frame, for per > 32 768
//   k_adam_step_frames        grid (blocks, F): k_adam_step on the rows of the frames that are active
//
// The early stop lives on the device: active_in[f] says whether frame f still optimises.  An inactive frame's grad is zeros (the
// backward pass through the batched UNet then does no work of consequence for it), its rec and loss are not touched, and the Adam
// step writes nothing of it.  Whichever thread writes loss[f] writes active_out[f] = active_in[f] && !((double)loss[f] <
// threshold), the reference's `loss.item() < epsilon + i * 2e-5` in float64: a loss at the threshold, or a NaN, does not stop.
// No atomics; nothing here waits for the device.
#include "cs_common.h"
#include "cs_ddimstep.h"
#include "cs_kernels.h"
#include "cs_latent.h"
#include "cs_nullloss.h"

namespace cs {

// thread 0 of the workgroup that finishes frame f's sum
__device__ __forceinline__ void frame_loss_and_flag(float hi, float lo, float count, double threshold, float* __restrict__ loss,
                                                    uint8_t* __restrict__ active_out, size_t f) {
    const float value = null_loss_mean(hi, lo, count);
    loss[f] = value;
    active_out[f] = (double)value < threshold ? 0 : 1;
}

template <class T, int PRED>
__global__ void __launch_bounds__(INV_THREADS) k_null_loss_grad_frames(
    const T* __restrict__ eps_uncond, const T* __restrict__ eps_cond, const T* __restrict__ latent_cur, const T* __restrict__ latent_prev,
    T* __restrict__ rec, T* __restrict__ grad, float* __restrict__ loss, float* __restrict__ partial,
    const uint8_t* __restrict__ active_in, uint8_t* __restrict__ active_out, size_t per, StepCoeffs k, double grad_scale, float count,
    double threshold) {
    __shared__ float sh_hi[INV_THREADS], sh_lo[INV_THREADS];
    const size_t f = blockIdx.y, base = f * per;
    if (!active_in[f]) {   // the whole workgroup takes this branch or none of it does
        const size_t begin = (size_t)blockIdx.x * INV_BLOCK_ELEMS;
        const size_t end = begin + INV_BLOCK_ELEMS < per ? begin + INV_BLOCK_ELEMS : per;
        for (size_t i = begin + threadIdx.x; i < end; i += INV_THREADS) grad[base + i] = (T)0.0f;
        if (gridDim.x == 1 && threadIdx.x == 0) active_out[f] = 0;
        return;
    }
    float hi = 0.0f, lo = 0.0f;
    null_loss_block<T, PRED>(eps_uncond + base, eps_cond + base, latent_cur + base, latent_prev + base, rec + base, grad + base,
                             blockIdx.x, per, k, grad_scale, hi, lo);
    block_reduce_pairs(hi, lo, sh_hi, sh_lo);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            frame_loss_and_flag(hi, lo, count, threshold, loss, active_out, f);
        } else {
            float* mine = partial + 2 * (f * gridDim.x + blockIdx.x);
            mine[0] = hi;
            mine[1] = lo;
        }
    }
}

__global__ void __launch_bounds__(INV_THREADS) k_null_loss_final_frames(const float* __restrict__ partial, int blocks,
                                                                        float* __restrict__ loss, const uint8_t* __restrict__ active_in,
                                                                        uint8_t* __restrict__ active_out, float count, double threshold) {
    __shared__ float sh_hi[INV_THREADS], sh_lo[INV_THREADS];
    const size_t f = blockIdx.x;
    if (!active_in[f]) {
        if (threadIdx.x == 0) active_out[f] = 0;
        return;
    }
    float hi = 0.0f, lo = 0.0f;
    null_loss_final_share(partial + 2 * f * (size_t)blocks, blocks, hi, lo);
    block_reduce_pairs(hi, lo, sh_hi, sh_lo);
    if (threadIdx.x == 0) frame_loss_and_flag(hi, lo, count, threshold, loss, active_out, f);
}

template <class T>
__global__ void __launch_bounds__(256) k_adam_step_frames(T* __restrict__ param, const T* __restrict__ grad, T* __restrict__ exp_avg,
                                                          T* __restrict__ exp_avg_sq, const uint8_t* __restrict__ active, size_t m,
                                                          AdamCoeffs k) {
    const size_t f = blockIdx.y, base = f * m;
    if (!active[f]) return;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += step) {
        adam_element<T>(param + base, grad + base, exp_avg + base, exp_avg_sq + base, i, k);
    }
}

size_t null_loss_frames_max() { return 65535; }   // the grid's second dimension

size_t null_loss_frames_workspace_bytes(size_t frames, size_t per) {
    const size_t blocks = null_loss_blocks(per);
    return blocks > 1 ? frames * blocks * 2 * sizeof(float) : 0;
}

hipError_t launch_null_loss_grad_frames(const void* eps_uncond, const void* eps_cond, const void* latent_cur, const void* latent_prev,
                                        void* rec, float* loss, void* grad, const uint8_t* active_in, uint8_t* active_out, int dtype,
                                        size_t frames, size_t per, float guidance, const float c[4], int prediction, double grad_scale,
                                        double threshold, void* workspace, hipStream_t stream) {
    const int blocks = (int)null_loss_blocks(per);
    const dim3 grid(blocks, (unsigned)frames), block(INV_THREADS);
    const StepCoeffs k{guidance, c[0], c[1], c[2], c[3]};
    float* partial = (float*)workspace;
    const float count = (float)per;
    with_latent_type(dtype, [&](auto tag) {
        using T = decltype(tag);
        with_prediction(prediction, [&](auto pred) {
            hipLaunchKernelGGL((k_null_loss_grad_frames<T, decltype(pred)::value>), grid, block, 0, stream, as<T>(eps_uncond),
                               as<T>(eps_cond), as<T>(latent_cur), as<T>(latent_prev), as<T>(rec), as<T>(grad), loss, partial, active_in,
                               active_out, per, k, grad_scale, count, threshold);
        });
    });
    if (blocks > 1)
        hipLaunchKernelGGL(k_null_loss_final_frames, dim3((unsigned)frames), block, 0, stream, partial, blocks, loss, active_in, active_out,
                           count, threshold);
    return hipGetLastError();
}

hipError_t launch_adam_step_frames(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, const uint8_t* active, int dtype,
                                   size_t frames, size_t m, const float k6[6], hipStream_t stream) {
    const AdamCoeffs k{k6[0], k6[1], k6[2], k6[3], k6[4], k6[5]};
    const dim3 grid(stream_grid(m), (unsigned)frames);
    with_latent_type(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(k_adam_step_frames<T>, grid, dim3(256), 0, stream, as<T>(param), as<T>(grad), as<T>(exp_avg), as<T>(exp_avg_sq),
                           active, m, k);
    });
    return hipGetLastError();
}

}  // namespace cs
