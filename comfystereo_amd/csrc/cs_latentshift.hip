// cs_latentshift.hip -- StereoDiffusion's Standard mode around its model (reference stereodiffusion_nodes.py:576-682): the latent
// shift as a plan made once per image and a per-step apply, and the decoded images' way to uint8 codes.
//
//   k_latent_shift_plan    the right view of stereo_shift_torch(shift_both=False) (reference stereo_utils.py:36-88) as a table:
//                          for every destination the source column the reference's sweep leaves there, -1 where nothing lands.
//                          The disparity does not change during the loop, so neither does the table.
//   k_latent_shift_apply   one launch per shift step, values moved and never computed (bit-exact in every dtype):
//                          FIRST (:650-660) gathers the right view, stores the mask `channel 0 != 0` and fills the holes with noise;
//                          RESHIFT (:663-667) gathers again where the stored mask is set.
//   k_decode_to_codes      (image / 2 + 0.5).clamp(0, 1), nan -> 0, * 255 in float32, truncated (:673-677), NCHW -> NHWC.
//
// No atomics: the plan's winner is found by scanning the sources within reach of a destination, highest (negative shift) or
// lowest (positive shift) first.
#include "cs_common.h"
#include "cs_kernels.h"
#include "cs_latent.h"

namespace cs {

// grid: (h, b).  dst[w] in LDS: the destination column of every source column of the row, -1 = it leaves the row.
// reach: no source lies further than this many columns from its destination.
__global__ void __launch_bounds__(256) k_latent_shift_plan(const float* __restrict__ depth, int h, int w, const uint32_t* stats,
                                                           float scale_px32, int asc, int reach, int pow_mode, float e32,
                                                           int32_t* __restrict__ src_col) {
    extern __shared__ int dst[];
    __shared__ csm::PowfTables T;
    const int row = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) { const csm::PowfTables init = CS_POWF_TABLES_INIT; T = init; }
    __syncthreads();
    const float mn = csm::ord2f(stats[ST_L_MIN]), mx = csm::ord2f(stats[ST_L_MAX]);
    const float rng = mx - mn;
    const bool flat = !(rng > 1.1920929e-07f);   // torch.finfo(float32).eps (stereo_utils.py:40)
    const float* drow = depth + ((size_t)b * h + row) * w;
    for (int col = tid; col < w; col += blockDim.x) {
        int cd;
        dst[col] = stereo_shift_dest(drow[col], mn, rng, flat, pow_mode, e32, scale_px32, col, w, &T, cd) ? cd : -1;
    }
    __syncthreads();
    int32_t* out = src_col + ((size_t)b * h + row) * w;
    for (int x = tid; x < w; x += blockDim.x) {
        int win = -1;
        if (asc) {   // negative shift: the sweep runs over ascending columns, the highest source is written last (:59-62)
            for (int col = min(x + reach, w - 1); col >= x; col--)
                if (dst[col] == x) { win = col; break; }
        } else {     // positive (or no) shift: descending columns, the lowest source is written last
            for (int col = max(x - reach, 0); col <= x; col++)
                if (dst[col] == x) { win = col; break; }
        }
        out[x] = win;
    }
}

hipError_t launch_latent_shift_plan(const float* depth, int b, int h, int w, const uint32_t* stats, double scale_px, double exponent,
                                    int32_t* src_col, hipStream_t stream) {
    // |normalised depth ^ e| <= 1 for e > 0, so |shift| <= |trunc(scale_px)|; any other exponent: the whole row
    const double mag = scale_px < 0 ? -scale_px : scale_px;
    const int reach = (exponent > 0.0 && mag < (double)(w - 1)) ? (int)mag + 1 : w - 1;
    hipLaunchKernelGGL(k_latent_shift_plan, dim3(h, b), dim3(256), (size_t)w * 4, stream, depth, h, w, stats, (float)scale_px,
                       scale_px < 0 ? 1 : 0, reach, stereo_shift_pow_mode(exponent), (float)exponent, src_col);
    return hipGetLastError();
}

// U: the element as an unsigned integer of its size (values are moved, never computed).  One thread per pixel (b, row, x), all
// channels.  The gather and the mask `channel 0 != 0`: shift_gathered and shift_mask of cs_latent.h, which k_standard_step shares.
template <class U>
__global__ void __launch_bounds__(256) k_latent_shift_apply(const U* __restrict__ left, U* __restrict__ right,
                                                            const int32_t* __restrict__ src_col, uint8_t* __restrict__ mask,
                                                            const U* __restrict__ noise, int c, int h, int w, size_t pixels, int op) {
    const size_t plane = (size_t)h * w, step = (size_t)gridDim.x * blockDim.x;
    for (size_t pix = blockIdx.x * (size_t)blockDim.x + threadIdx.x; pix < pixels; pix += step) {
        const size_t br = pix / w;
        const int x = (int)(pix - br * w);
        const size_t bb = br / h, r = br - bb * h;
        const size_t base = (bb * c * h + r) * w;   // (b, channel 0, row, column 0)
        const int src = src_col[pix];
        const bool landed = shift_landed(src, w);
        const auto gathered = [&](int ch) { return shift_gathered(landed, left, base + ch * plane + src); };
        if (op == CS_LATENT_FIRST) {
            const U v0 = gathered(0);
            const bool m = shift_mask(v0);
            mask[pix] = m ? 1 : 0;
            if (noise && !m) {
                for (int ch = 0; ch < c; ch++) right[base + ch * plane + x] = noise[base + ch * plane + x];
            } else {
                right[base + x] = v0;
                for (int ch = 1; ch < c; ch++) right[base + ch * plane + x] = gathered(ch);
            }
        } else if (mask[pix]) {
            for (int ch = 0; ch < c; ch++) right[base + ch * plane + x] = gathered(ch);
        }
    }
}

hipError_t launch_latent_shift_apply(const void* left, void* right, const int32_t* src_col, uint8_t* mask, const void* noise,
                                     int dtype, int b, int c, int h, int w, int op, hipStream_t stream) {
    const size_t pixels = (size_t)b * h * w;
    with_latent_type(dtype, [&](auto tag) {
        using U = typename BitsOf<sizeof(tag)>::type;   // float16 and bfloat16: one instantiation
        hipLaunchKernelGGL(k_latent_shift_apply<U>, dim3(stream_grid(pixels)), dim3(256), 0, stream, as<U>(left), as<U>(right), src_col,
                           mask, as<U>(noise), c, h, w, pixels, op);
    });
    return hipGetLastError();
}

// (x / 2 + 0.5) as torch computes it on a tensor of type T: the quotient rounded to T, then the sum rounded to T.
//   float32: two IEEE operations.
//   half types: the widened x times 0.5 is exact in float32, so the conversion back is the quotient's one rounding.  The sum of
//   that and 0.5 is formed in float64, brought to float32 by rounding to odd (truncate, then set the last bit if anything was
//   lost) and converted to T: with 13 or more spare bits in between, rounding to odd followed by rounding to nearest is
//   rounding the float64 sum to T once.  The float64 sum itself is exact wherever the result matters: a quotient in
//   [-0.5, 0.5] with a last bit of 2^-40 or more; a smaller one rounds to 0.5 through any path, and a sum outside [0, 1]
//   stays outside under any monotonic rounding and is clamped.
template <class T>
__device__ __forceinline__ float half_plus_half(T x) {
    const T q = (T)((float)x * 0.5f);
    const double s = (double)(float)q + 0.5;
    float f = (float)s;
    if (s == s && (double)f != s) {   // inexact (s is finite here: a float plus 0.5)
        uint32_t u = csm::f2u(f);
        const double a = (double)f;
        if ((a < 0 ? -a : a) > (s < 0 ? -s : s)) u -= 1;   // the conversion rounded away from zero: step back
        f = csm::u2f(u | 1u);
    }
    return (float)(T)f;
}
template <>
__device__ __forceinline__ float half_plus_half<float>(float x) {
    const float q = x * 0.5f;   // = x / 2, rounded once
    return q + 0.5f;
}

template <class T>
__global__ void __launch_bounds__(256) k_decode_to_codes(const T* __restrict__ image, int c, size_t hw, size_t pixels,
                                                         uint8_t* __restrict__ codes) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    for (size_t pix = blockIdx.x * (size_t)blockDim.x + threadIdx.x; pix < pixels; pix += step) {
        const size_t nn = pix / hw, p = pix - nn * hw;
        for (int ch = 0; ch < c; ch++) {
            const float s = half_plus_half<T>(image[(nn * c + ch) * hw + p]);
            // clamp(0, 1) keeps a NaN, nan_to_num makes it 0 (:673-676); the product is float32, the conversion truncates (:677)
            const float v = (s == s) ? fminf(fmaxf(s, 0.0f), 1.0f) : 0.0f;
            codes[pix * c + ch] = (uint8_t)(int)(v * 255.0f);
        }
    }
}

hipError_t launch_decode_to_codes(const void* image, int dtype, int n, int c, int h, int w, uint8_t* codes, hipStream_t stream) {
    const size_t hw = (size_t)h * w, pixels = (size_t)n * hw;
    with_latent_type(dtype, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL(k_decode_to_codes<T>, dim3(stream_grid(pixels)), dim3(256), 0, stream, as<T>(image), c, hw, pixels, codes);
    });
    return hipGetLastError();
}

}  // namespace cs
