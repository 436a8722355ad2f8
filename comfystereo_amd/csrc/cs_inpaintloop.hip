// cs_inpaintloop.hip -- StereoDiffusion's Fast mode outside its models (reference model_wrappers.py ComfyUIInpaintRunner.__call__,
// :522-641): the tensor work before and inside the denoising loop, around one persistent UNet input
//   x [2n][9][hl][wl]   uncond half, then cond half (torch.cat([latent_model_input] * 2), :610); per frame: latents (channels 0..3),
//                       the mask at the latents' size (4), the masked image's latents (5..8) (:607)
//
//   k_inpaint_image_prep    codes and mask -> img, img * (1 - mask) (:562-572), F.interpolate(mask, "nearest") into channel 4 (:580)
//   k_inpaint_latent_init   mean * 0.18215 twice (:575-576, :583-584), scheduler.add_noise (:600) -> channels 0..3 and 5..8
//   k_inpaint_plms_step     guidance (:622) and one PLMS step (:625) in one launch: the new latents go straight into channels 0..3
//                           of both halves, the prediction into the history slot the host names, latents / 0.18215 (:628) on request
//
// Arithmetic, as cs_inversion.hip: every operation of the reference's tensor expression is one operation here, rounded once to the
// tensors' dtype before the next -- float32: plain IEEE (the library is built with -ffp-contract=off); float16 / bfloat16: the
// operation in float32, then the conversion.  Every operand is elementwise: no LDS, no atomics.  16-byte accesses where the
// pointers and hl * wl (h * w) allow, one element (pixel) per access otherwise.
#include "cs_common.h"
#include "cs_ddimstep.h"
#include "cs_kernels.h"
#include "cs_latent.h"

namespace cs {

namespace {

// rnd<T>(x), x rounded to T as a float, mul_rnd<T>(a, b), a product rounded to float32 and then to T as CPU torch rounds it
// (the empty asm that keeps the compiler from folding it into v_fma_mixlo_f16), and guided<T>, the
// guidance (:622): cs_ddimstep.h, the one definition, shared with cs_inversion.hip and cs_standardloop.hip.  Chunk, load and
// store, the 16-byte access: cs_latent.h.

constexpr float VAE_SCALE = 0.18215f;   // the Python scalar 0.18215 as torch hands it to a float32 operation

}  // namespace

// ---- 1. codes and mask -> img, masked, the mask at the latents' size -------------------------------------------------------------
// P pixels per thread.  filled [n][h][w][3] uint8, mask [n][h][w] uint8 -> img, masked [n][3][h][w] of T; then, in the same launch,
// x[frame][4] and x[n + frame][4] = mask[nearest].  pixels = n * h * w, a multiple of P per frame when P > 1.
template <class T, int P>
__global__ void __launch_bounds__(256) k_inpaint_image_prep(const uint8_t* __restrict__ filled, const uint8_t* __restrict__ mask,
                                                            T* __restrict__ img, T* __restrict__ masked, T* __restrict__ x, int n, int h,
                                                            int w, int hl, int wl, float scale_h, float scale_w) {
    const size_t hw = (size_t)h * w, pixels = (size_t)n * hw, step = (size_t)gridDim.x * blockDim.x;
    const size_t first = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    for (size_t j = first; j < pixels / P; j += step) {
        const size_t pix = j * P, frame = pix / hw, p = pix - frame * hw;
        uint8_t codes[3 * P], m[P];
        if constexpr (P == 1) {
            for (int k = 0; k < 3; k++) codes[k] = filled[pix * 3 + k];
            m[0] = mask[pix];
        } else {   // 3 P and P bytes as 32-bit words (P is a multiple of 4, the pointers are aligned)
            const uint32_t* cw = reinterpret_cast<const uint32_t*>(filled + pix * 3);
            const uint32_t* mw = reinterpret_cast<const uint32_t*>(mask + pix);
#pragma unroll
            for (int k = 0; k < 3 * P / 4; k++) {
                const uint32_t word = cw[k];
                for (int b = 0; b < 4; b++) codes[4 * k + b] = (uint8_t)(word >> (8 * b));
            }
#pragma unroll
            for (int k = 0; k < P / 4; k++) {
                const uint32_t word = mw[k];
                for (int b = 0; b < 4; b++) m[4 * k + b] = (uint8_t)(word >> (8 * b));
            }
        }
        Chunk<T, P> o_img[3], o_masked[3];
#pragma unroll
        for (int k = 0; k < P; k++) {
            const float keep = rnd<T>(1.0f - (m[k] ? 1.0f : 0.0f));   // 1 - mask_t, in T (:572)
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                // (code / 255.0 in float32, :562; * 2.0 - 1.0 in float32, then the conversion, :564)
                const float v = rnd<T>(((float)codes[3 * k + ch] / 255.0f) * 2.0f - 1.0f);
                o_img[ch].v[k] = (T)v;
                o_masked[ch].v[k] = (T)mul_rnd<T>(v, keep);   // a negative pixel under the mask: -0.0
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            store<T, P>(img + (frame * 3 + ch) * hw + p, o_img[ch]);
            store<T, P>(masked + (frame * 3 + ch) * hw + p, o_masked[ch]);
        }
    }
    // torch's nearest source index: floor(dst * scale) in float32, at most the last (UpSample.h nearest_neighbor_compute_source_index)
    const size_t hwl = (size_t)hl * wl, cells = (size_t)n * hwl;
    for (size_t j = first; j < cells; j += step) {
        const size_t frame = j / hwl, q = j - frame * hwl;
        const int y = (int)(q / wl), xq = (int)(q - (size_t)y * wl);
        int sy = (int)floorf((float)y * scale_h), sx = (int)floorf((float)xq * scale_w);
        sy = sy < h - 1 ? sy : h - 1;
        sx = sx < w - 1 ? sx : w - 1;
        const T v = (T)(mask[frame * hw + (size_t)sy * w + sx] ? 1.0f : 0.0f);
        x[(frame * 9 + 4) * hwl + q] = v;
        x[((frame + n) * 9 + 4) * hwl + q] = v;
    }
}

// ---- 2. the two VAE means -> the image latents, the first latents, the masked image's latents -------------------------------------
// M: the dtype the VAE returned, T: the model's.  per = 4 * hl * wl elements per frame, total = n * per, both multiples of W.
template <class M, class T, int W>
__global__ void __launch_bounds__(256) k_inpaint_latent_init(const M* __restrict__ mean_img, const M* __restrict__ mean_masked,
                                                             const T* __restrict__ noise, T* __restrict__ x, T* __restrict__ img_latent,
                                                             T* __restrict__ decode_in, size_t per, size_t total, size_t half_stride, float sa, float sb) {
    const size_t step = (size_t)gridDim.x * blockDim.x, frame_stride = per / 4 * 9;
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < total / W; j += step) {
        const size_t i = j * W, frame = i / per, xoff = frame * frame_stride + (i - frame * per);
        const Chunk<M, W> a = load<M, W>(mean_img + i), b = load<M, W>(mean_masked + i);
        Chunk<T, W> nz, lat, il, ml, dec;
        if (noise) nz = load<T, W>(noise + i);
#pragma unroll
        for (int k = 0; k < W; k++) {
            // mean * 0.18215 in the mean's dtype (:575-576), then .to(model_dtype) (:583-584)
            const float li = rnd<T>(mul_rnd<M>((float)a.v[k], VAE_SCALE)), lm = rnd<T>(mul_rnd<M>((float)b.v[k], VAE_SCALE));
            il.v[k] = (T)li;
            ml.v[k] = (T)lm;
            // add_noise (:600): sa * img_latent + sb * noise; no timestep (:602): img_latent
            const float l0 = noise ? rnd<T>(mul_rnd<T>(sa, li) + mul_rnd<T>(sb, (float)nz.v[k])) : li;
            lat.v[k] = (T)l0;
            dec.v[k] = (T)(l0 / VAE_SCALE);   // (:628)
        }
        store<T, W>(img_latent + i, il);
        if (decode_in) store<T, W>(decode_in + i, dec);
        store<T, W>(x + xoff, lat);
        store<T, W>(x + half_stride + xoff, lat);
        store<T, W>(x + xoff + per / 4 * 5, ml);
        store<T, W>(x + half_stride + xoff + per / 4 * 5, ml);
    }
}

// ---- 3. guidance and one PLMS step ----------------------------------------------------------------------------------------------
struct PlmsCoeffs {
    float guidance, sc, da, denom;
    int kind;
};

// the linear multistep combination of this step's prediction e with the earlier ones e1 (the latest) .. e3
template <class T>
__device__ __forceinline__ float plms_combine(int kind, float e, float e1, float e2, float e3) {
    switch (kind) {
    case CS_PLMS_FIRST: return e;
    case CS_PLMS_SECOND: return rnd<T>(rnd<T>(e + e1) / 2.0f);
    case CS_PLMS_ORDER2: return rnd<T>(rnd<T>(mul_rnd<T>(3.0f, e) - e1) / 2.0f);
    case CS_PLMS_ORDER3: return rnd<T>(rnd<T>(rnd<T>(mul_rnd<T>(23.0f, e) - mul_rnd<T>(16.0f, e1)) + mul_rnd<T>(5.0f, e2)) / 12.0f);
    default: {
        const float s = rnd<T>(rnd<T>(rnd<T>(mul_rnd<T>(55.0f, e) - mul_rnd<T>(59.0f, e1)) + mul_rnd<T>(37.0f, e2)) - mul_rnd<T>(9.0f, e3));
        return mul_rnd<T>((float)(1.0 / 24.0), s);
    }
    }
}

// noise_pred [2n][4][hl][wl]; x as above; e_out, e1..e3, cur_sample, decode_in [n][4][hl][wl].  x's first half is read (the sample,
// unless the kind takes it from cur_sample) and written by the same thread, element by element.
template <class T, int W>
__global__ void __launch_bounds__(256) k_inpaint_plms_step(const T* __restrict__ noise_pred, T* x, T* __restrict__ e_out,
                                                           const T* __restrict__ e1, const T* __restrict__ e2, const T* __restrict__ e3,
                                                           T* cur_sample, T* __restrict__ decode_in, size_t per, size_t total,
                                                           size_t half_stride, PlmsCoeffs k) {
    const size_t step = (size_t)gridDim.x * blockDim.x, frame_stride = per / 4 * 9;
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < total / W; j += step) {
        const size_t i = j * W, frame = i / per, xoff = frame * frame_stride + (i - frame * per);
        const Chunk<T, W> u = load<T, W>(noise_pred + i), t = load<T, W>(noise_pred + total + i);
        const Chunk<T, W> s = k.kind == CS_PLMS_SECOND ? load<T, W>(cur_sample + i) : load<T, W>(x + xoff);
        Chunk<T, W> h1 = {}, h2 = {}, h3 = {};
        if (k.kind >= CS_PLMS_SECOND) h1 = load<T, W>(e1 + i);
        if (k.kind >= CS_PLMS_ORDER3) h2 = load<T, W>(e2 + i);
        if (k.kind >= CS_PLMS_ORDER4) h3 = load<T, W>(e3 + i);
        Chunk<T, W> e_c, prev_c, dec_c;
#pragma unroll
        for (int q = 0; q < W; q++) {
            const float e = guided<T>((float)u.v[q], (float)t.v[q], true, k.guidance);   // (:622)
            const float m = plms_combine<T>(k.kind, e, (float)h1.v[q], (float)h2.v[q], (float)h3.v[q]);
            // sc * sample - da * m / denom
            const float prev = rnd<T>(mul_rnd<T>(k.sc, (float)s.v[q]) - rnd<T>(mul_rnd<T>(k.da, m) / k.denom));
            e_c.v[q] = (T)e;
            prev_c.v[q] = (T)prev;
            dec_c.v[q] = (T)(prev / VAE_SCALE);   // (:628)
        }
        if (k.kind == CS_PLMS_FIRST) store<T, W>(cur_sample + i, s);
        if (k.kind != CS_PLMS_SECOND) store<T, W>(e_out + i, e_c);
        store<T, W>(x + xoff, prev_c);
        store<T, W>(x + half_stride + xoff, prev_c);
        if (decode_in) store<T, W>(decode_in + i, dec_c);
    }
}

template <class T>
static void image_prep(const uint8_t* filled, const uint8_t* mask, void* img, void* masked, void* x, int n, int h, int w, int hl, int wl,
                       hipStream_t stream) {
    constexpr int P = 16 / sizeof(T);
    const size_t hw = (size_t)h * w, pixels = (size_t)n * hw, cells = (size_t)n * hl * wl;
    const float scale_h = (float)h / (float)hl, scale_w = (float)w / (float)wl;   // torch's compute_scales_value<float>
    // whole chunks per frame and per plane; the codes and the mask are read as 16-, 8- or 4-byte words
    const bool wide = hw % P == 0 && aligned16({filled, mask, img, masked});
    const size_t items = wide ? (pixels / P > cells ? pixels / P : cells) : (pixels > cells ? pixels : cells);
    launch_wide_or_narrow(wide, k_inpaint_image_prep<T, P>, k_inpaint_image_prep<T, 1>, dim3(stream_grid(items)), dim3(256), 0, stream,
                          filled, mask, as<T>(img), as<T>(masked), as<T>(x), n, h, w, hl, wl, scale_h, scale_w);
}

hipError_t launch_inpaint_image_prep(const uint8_t* filled, const uint8_t* mask, int n, int h, int w, int hl, int wl, int dtype, void* img,
                                     void* masked, void* x, hipStream_t stream) {
    with_latent_type(dtype, [&](auto tag) { image_prep<decltype(tag)>(filled, mask, img, masked, x, n, h, w, hl, wl, stream); });
    return hipGetLastError();
}

// M: the means' type, T: the model's
template <class M, class T>
static void latent_init(const void* mean_img, const void* mean_masked, const void* noise, void* x, void* img_latent, void* decode_in,
                        int n, size_t hwl, float sa, float sb, hipStream_t stream) {
    constexpr int W = 16 / sizeof(T);
    const size_t per = 4 * hwl, total = (size_t)n * per, half_stride = (size_t)n * 9 * hwl;
    const bool wide = hwl % W == 0 && aligned16({mean_img, mean_masked, noise, x, img_latent, decode_in});
    launch_wide_or_narrow(wide, k_inpaint_latent_init<M, T, W>, k_inpaint_latent_init<M, T, 1>, dim3(stream_grid(wide ? total / W : total)),
                          dim3(256), 0, stream, as<M>(mean_img), as<M>(mean_masked), as<T>(noise), as<T>(x), as<T>(img_latent),
                          as<T>(decode_in), per, total, half_stride, sa, sb);
}

hipError_t launch_inpaint_latent_init(const void* mean_img, const void* mean_masked, int mean_dtype, const void* noise, int dtype, int n,
                                      int hl, int wl, float sa, float sb, void* x, void* img_latent, void* decode_in, hipStream_t stream) {
    const size_t hwl = (size_t)hl * wl;
    with_latent_type(mean_dtype, [&](auto mean_tag) {
        with_latent_type(dtype, [&](auto tag) {
            latent_init<decltype(mean_tag), decltype(tag)>(mean_img, mean_masked, noise, x, img_latent, decode_in, n, hwl, sa, sb, stream);
        });
    });
    return hipGetLastError();
}

template <class T>
static void plms_step(const void* noise_pred, void* x, void* e_out, const void* e1, const void* e2, const void* e3, void* cur_sample,
                      void* decode_in, int n, size_t hwl, const PlmsCoeffs& k, hipStream_t stream) {
    constexpr int W = 16 / sizeof(T);
    const size_t per = 4 * hwl, total = (size_t)n * per, half_stride = (size_t)n * 9 * hwl;
    const bool wide = hwl % W == 0 && aligned16({noise_pred, x, e_out, e1, e2, e3, cur_sample, decode_in});
    launch_wide_or_narrow(wide, k_inpaint_plms_step<T, W>, k_inpaint_plms_step<T, 1>, dim3(stream_grid(wide ? total / W : total)), dim3(256),
                          0, stream, as<T>(noise_pred), as<T>(x), as<T>(e_out), as<T>(e1), as<T>(e2), as<T>(e3), as<T>(cur_sample),
                          as<T>(decode_in), per, total, half_stride, k);
}

hipError_t launch_inpaint_plms_step(const void* noise_pred, void* x, int dtype, int n, int hl, int wl, int kind, float guidance, float sc,
                                    float da, float denom, void* e_out, const void* e1, const void* e2, const void* e3, void* cur_sample,
                                    void* decode_in, hipStream_t stream) {
    const PlmsCoeffs k{guidance, sc, da, denom, kind};
    const size_t hwl = (size_t)hl * wl;
    with_latent_type(dtype, [&](auto tag) { plms_step<decltype(tag)>(noise_pred, x, e_out, e1, e2, e3, cur_sample, decode_in, n, hwl, k, stream); });
    return hipGetLastError();
}

}  // namespace cs
