// cs_fewstep.hip -- Fast mode's denoising loop for few-step models (SD-Turbo, LCM checkpoints), outside the models: the samplers a
// distilled model was trained for, each step one launch around the persistent UNet input of cs_inpaintloop.hip
//   x [2n or n][C][hl][wl]   C = 9: an inpainting UNet (latents, mask, masked image's latents; channels 4..8 written once before the
//                            loop); C = 4: an ordinary UNet used RePaint-style -- outside the mask the latents are replaced after
//                            every step by the image's latents at the next noise level.  With classifier-free guidance the uncond
//                            half, then the cond half; without it (guidance_scale <= 1) the conditional batch alone.
//
//   k_inpaint_fewstep_init   the first latents from the image's latents and the initial noise (Euler: the un-scaled sample into
//                            `state`, the scaled one into x; LCM: scheduler.add_noise), the mask at the latents' size for C = 4
//   k_inpaint_fewstep_step   guidance, one Euler step (Karras et al. 2022, Alg. 1 without churn) or one multistep consistency
//                            sampling step (Luo et al. 2023), the blend for C = 4, latents / 0.18215 on request
//
// Arithmetic (the specification is tools/fewstep_oracle.py, CPU torch): the guided prediction e is formed in the tensors' dtype as
// everywhere (guided<T>, cs_ddimstep.h); the rest of a step is float32 arithmetic on the dtype's values with float32 coefficients
// from the host, one IEEE operation each (the library is built with -ffp-contract=off; f32() below keeps every result a value of its
// own, so that no operation is folded into a conversion), and one rounding to the dtype per stored
// tensor.  Elementwise: no LDS, no atomics.  16-byte accesses where the pointers and hl * wl allow, one element per access otherwise.
#include "cs_common.h"
#include "cs_ddimstep.h"
#include "cs_kernels.h"
#include "cs_latent.h"

namespace cs {

namespace {

constexpr float VAE_SCALE = 0.18215f;   // the Python scalar 0.18215 as a float32

// a float32 result as a value of its own (mul_rnd's empty asm, for any operation)
__device__ __forceinline__ float f32(float v) {
    asm("" : "+v"(v));
    return v;
}

struct FewstepCoeffs {
    float guidance, k[6];
    int last;
};

// the sample after one step, in float32, from the sample s, the guided prediction e and (LCM, not the last step) fresh noise z
//   Euler  k0 = sigma_next - sigma_t:                                  s + e * k0                                  (2 roundings)
//   LCM    k0 = sqrt(1 - a_t), k1 = sqrt(a_t), k2 = c_out, k3 = c_skip, k4 = sqrt(a_next), k5 = sqrt(1 - a_next):
//          x0 = (s - k0 * e) / k1; den = k2 * x0 + k3 * s; k4 * den + k5 * z, on the last step den   (9 roundings, 6 on the last)
template <int SAMPLER>
__device__ __forceinline__ float fewstep_prev(float s, float e, float z, const FewstepCoeffs& c) {
    if constexpr (SAMPLER == CS_FEWSTEP_EULER) return f32(s + f32(e * c.k[0]));
    const float x0 = f32(f32(s - f32(c.k[0] * e)) / c.k[1]);
    const float den = f32(f32(c.k[2] * x0) + f32(c.k[3] * s));
    return c.last ? den : f32(f32(c.k[4] * den) + f32(c.k[5] * z));
}

// the image's latents at the next noise level, in float32 (C = 4, outside the mask); on the last step the image's latents
//   Euler  k2 = sigma_next:  il + k2 * noise0          LCM  k4 * il + k5 * noise0
template <int SAMPLER>
__device__ __forceinline__ float fewstep_keep(float il, float nz, const FewstepCoeffs& c) {
    if (c.last) return il;
    if constexpr (SAMPLER == CS_FEWSTEP_EULER) return f32(il + f32(c.k[2] * nz));
    return f32(f32(c.k[4] * il) + f32(c.k[5] * nz));
}

}  // namespace

// ---- 1. the first latents -------------------------------------------------------------------------------------------------------
// img_latent, noise, state [n][4][hl][wl]; x [halves * n][C][hl][wl]; C = 4: mask_l [n][hl][wl] = channel 4 of x9 [2n][9][hl][wl]
// (what k_inpaint_image_prep wrote there).  per = 4 * hl * wl, total = n * per, both multiples of W.
//   Euler  k0 = sigma_0, k1 = sqrt(sigma_0^2 + 1):  state = il + k0 * noise (float32, rounded once); x = that / k1 (rounded once)
//   LCM    k0, k1 = scheduler.add_noise's two roots in the dtype:  x = k0 * il + k1 * noise, every operation rounded to the dtype
//   no noise (no timestep left): x = il
template <class T, int W>
__global__ void __launch_bounds__(256) k_inpaint_fewstep_init(const T* __restrict__ img_latent, const T* __restrict__ noise,
                                                              const T* __restrict__ x9, T* __restrict__ x, T* __restrict__ state,
                                                              T* __restrict__ mask_l, size_t per, size_t total, int channels, int halves,
                                                              int sampler, float k0, float k1) {
    const size_t step = (size_t)gridDim.x * blockDim.x, hwl = per / 4, frame_stride = hwl * channels, half_stride = total / 4 * channels;
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < total / W; j += step) {
        const size_t i = j * W, frame = i / per, r = i - frame * per, xoff = frame * frame_stride + r;
        const Chunk<T, W> il = load<T, W>(img_latent + i);
        Chunk<T, W> nz = {}, st, xv;
        if (noise) nz = load<T, W>(noise + i);
#pragma unroll
        for (int q = 0; q < W; q++) {
            const float li = (float)il.v[q], ns = (float)nz.v[q];
            if (!noise) {
                st.v[q] = il.v[q];
                xv.v[q] = il.v[q];
            } else if (sampler == CS_FEWSTEP_EULER) {
                const float lat = f32(li + f32(k0 * ns));
                st.v[q] = (T)lat;
                xv.v[q] = (T)f32(lat / k1);
            } else {
                const float lat = rnd<T>(mul_rnd<T>(k0, li) + mul_rnd<T>(k1, ns));
                st.v[q] = (T)lat;
                xv.v[q] = (T)lat;
            }
        }
        store<T, W>(x + xoff, xv);
        if (halves == 2) store<T, W>(x + half_stride + xoff, xv);
        if (state) store<T, W>(state + i, st);
        if (mask_l && r < hwl) store<T, W>(mask_l + frame * hwl + r, load<T, W>(x9 + (frame * 9 + 4) * hwl + r));
    }
}

// ---- 2. guidance and one step ---------------------------------------------------------------------------------------------------
// noise_pred [2n or n][4][hl][wl] (CFG: uncond, cond); x as above; state (Euler: the un-scaled sample, read and written), z (LCM, not
// the last step: this step's noise), img_latent, noise0 (C = 4), decode_in [n][4][hl][wl]; mask_l [n][hl][wl] (C = 4).  LCM reads
// the sample from x's first half, which the same thread writes, element by element.
template <class T, int W, int SAMPLER, bool CFG, int C>
__global__ void __launch_bounds__(256) k_inpaint_fewstep_step(const T* __restrict__ noise_pred, T* x, T* state, const T* __restrict__ z,
                                                              const T* __restrict__ img_latent, const T* __restrict__ noise0,
                                                              const T* __restrict__ mask_l, T* __restrict__ decode_in, size_t per,
                                                              size_t total, FewstepCoeffs c) {
    const size_t step = (size_t)gridDim.x * blockDim.x, hwl = per / 4, frame_stride = hwl * C, half_stride = total / 4 * C;
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < total / W; j += step) {
        const size_t i = j * W, frame = i / per, r = i - frame * per, xoff = frame * frame_stride + r;
        const Chunk<T, W> u = load<T, W>(noise_pred + i);
        Chunk<T, W> t = {}, zs = {}, il = {}, nz = {}, m = {};
        if constexpr (CFG) t = load<T, W>(noise_pred + total + i);
        const Chunk<T, W> s = SAMPLER == CS_FEWSTEP_EULER ? load<T, W>(state + i) : load<T, W>(x + xoff);
        if (SAMPLER == CS_FEWSTEP_LCM && !c.last) zs = load<T, W>(z + i);
        if constexpr (C == 4) {
            il = load<T, W>(img_latent + i);
            if (!c.last) nz = load<T, W>(noise0 + i);
            m = load<T, W>(mask_l + frame * hwl + r % hwl);   // (a chunk stays within one channel: hwl is a multiple of W)
        }
        Chunk<T, W> x_c, st_c, dec_c;
#pragma unroll
        for (int q = 0; q < W; q++) {
            const float e = guided<T>((float)u.v[q], (float)t.v[q], CFG, c.guidance);
            float lat = fewstep_prev<SAMPLER>((float)s.v[q], e, (float)zs.v[q], c);
            if constexpr (C == 4) {   // a select: the value of one side is moved, nothing is multiplied by the mask
                const float keep = fewstep_keep<SAMPLER>((float)il.v[q], (float)nz.v[q], c);
                lat = (float)m.v[q] != 0.0f ? lat : keep;
            }
            st_c.v[q] = (T)lat;
            // Euler: the next step's scale_model_input, k1 = sqrt(sigma_next^2 + 1) (1 on the last step)
            x_c.v[q] = SAMPLER == CS_FEWSTEP_EULER ? (T)f32(lat / c.k[1]) : (T)lat;
            dec_c.v[q] = (T)f32(lat / VAE_SCALE);
        }
        if constexpr (SAMPLER == CS_FEWSTEP_EULER) store<T, W>(state + i, st_c);
        store<T, W>(x + xoff, x_c);
        if constexpr (CFG) store<T, W>(x + half_stride + xoff, x_c);
        if (decode_in) store<T, W>(decode_in + i, dec_c);
    }
}

template <class T>
static void fewstep_init(const void* img_latent, const void* noise, const void* x9, void* x, void* state, void* mask_l, int n, size_t hwl,
                         int channels, int halves, int sampler, float k0, float k1, hipStream_t stream) {
    constexpr int W = 16 / sizeof(T);
    const size_t per = 4 * hwl, total = (size_t)n * per;
    const bool wide = hwl % W == 0 && aligned16({img_latent, noise, x9, x, state, mask_l});
    launch_wide_or_narrow(wide, k_inpaint_fewstep_init<T, W>, k_inpaint_fewstep_init<T, 1>, dim3(stream_grid(wide ? total / W : total)),
                          dim3(256), 0, stream, as<T>(img_latent), as<T>(noise), as<T>(x9), as<T>(x), as<T>(state), as<T>(mask_l), per, total,
                          channels, halves, sampler, k0, k1);
}

hipError_t launch_inpaint_fewstep_init(const void* img_latent, const void* noise, const void* x9, int dtype, int n, int hl, int wl,
                                       int channels, int halves, int sampler, float k0, float k1, void* x, void* state, void* mask_l,
                                       hipStream_t stream) {
    const size_t hwl = (size_t)hl * wl;
    with_latent_type(dtype, [&](auto tag) {
        fewstep_init<decltype(tag)>(img_latent, noise, x9, x, state, mask_l, n, hwl, channels, halves, sampler, k0, k1, stream);
    });
    return hipGetLastError();
}

template <class T, int SAMPLER, bool CFG, int C>
static void fewstep_step(const void* noise_pred, void* x, void* state, const void* z, const void* img_latent, const void* noise0,
                         const void* mask_l, void* decode_in, int n, size_t hwl, const FewstepCoeffs& c, hipStream_t stream) {
    constexpr int W = 16 / sizeof(T);
    const size_t per = 4 * hwl, total = (size_t)n * per;
    const bool wide = hwl % W == 0 && aligned16({noise_pred, x, state, z, img_latent, noise0, mask_l, decode_in});
    launch_wide_or_narrow(wide, k_inpaint_fewstep_step<T, W, SAMPLER, CFG, C>, k_inpaint_fewstep_step<T, 1, SAMPLER, CFG, C>,
                          dim3(stream_grid(wide ? total / W : total)), dim3(256), 0, stream, as<T>(noise_pred), as<T>(x), as<T>(state),
                          as<T>(z), as<T>(img_latent), as<T>(noise0), as<T>(mask_l), as<T>(decode_in), per, total, c);
}

// the instantiation of (sampler, cfg, channels), all checked by the caller
template <class T, class... Args>
static void fewstep_dispatch(int sampler, bool cfg, int channels, Args... args) {
    const int which = (sampler == CS_FEWSTEP_LCM ? 4 : 0) + (cfg ? 2 : 0) + (channels == 4 ? 1 : 0);
    switch (which) {
    case 0: return fewstep_step<T, CS_FEWSTEP_EULER, false, 9>(args...);
    case 1: return fewstep_step<T, CS_FEWSTEP_EULER, false, 4>(args...);
    case 2: return fewstep_step<T, CS_FEWSTEP_EULER, true, 9>(args...);
    case 3: return fewstep_step<T, CS_FEWSTEP_EULER, true, 4>(args...);
    case 4: return fewstep_step<T, CS_FEWSTEP_LCM, false, 9>(args...);
    case 5: return fewstep_step<T, CS_FEWSTEP_LCM, false, 4>(args...);
    case 6: return fewstep_step<T, CS_FEWSTEP_LCM, true, 9>(args...);
    default: return fewstep_step<T, CS_FEWSTEP_LCM, true, 4>(args...);
    }
}

hipError_t launch_inpaint_fewstep_step(const void* noise_pred, void* x, int dtype, int n, int hl, int wl, int channels, int sampler, int cfg,
                                       int last, float guidance, const float k[6], void* state, const void* step_noise,
                                       const void* img_latent, const void* noise0, const void* mask_l, void* decode_in, hipStream_t stream) {
    FewstepCoeffs c{guidance, {k[0], k[1], k[2], k[3], k[4], k[5]}, last};
    const size_t hwl = (size_t)hl * wl;
    with_latent_type(dtype, [&](auto tag) {
        fewstep_dispatch<decltype(tag)>(sampler, cfg != 0, channels, noise_pred, x, state, step_noise, img_latent, noise0, mask_l, decode_in,
                                        n, hwl, c, stream);
    });
    return hipGetLastError();
}

}  // namespace cs
