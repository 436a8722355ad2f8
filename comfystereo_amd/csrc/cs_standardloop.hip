// cs_standardloop.hip -- StereoDiffusion's Standard mode between two UNet calls (reference stereodiffusion_nodes.py:624-667 with
// diffusion_utils.diffusion_step :29-66) in one launch, around one persistent UNet input
//   x [4B][C][h][w]   rows 0..B-1 the left views, B..2B-1 the right views (the current latents), 2B..4B-1 their copy for the
//                     conditional half (torch.cat([latents] * 2))
//
//   k_standard_step   e = u + guidance * (c - u), the DDIM step (PRED: of an epsilon or a v-prediction model), then by `op` what
//                     k_latent_shift_apply does to the pair (new left, new right); the result goes into both halves of x.
//
// Arithmetic: cs_ddimstep.h, the statement cs_ddim_step uses -- the results are the bits of cs_ddim_step on the two halves
// followed by cs_latent_shift_apply.  The shift moves values and never computes.
//
// The in-place hazard: the right view at column j takes the NEW left value at column src_col[j], of its channel and of channel
// 0, while the left view's own thread overwrites x there.  One workgroup owns the rows (b, row) of every channel of both views.
// Phase A computes the new left values of the whole row -- every segment of it -- for a group of channels, stores them to x
// and keeps them in LDS; after the barrier phase B gathers from LDS only, never from x.  Nothing depends on the order in which
// workgroups or launches run.  A group is as many channels as fit the LDS budget (all of them at the latents' sizes); a later
// group reads the mask the first one stored, from global memory, behind the barrier between the groups.
// No atomics.  16-byte accesses where w and the pointers allow, one element per access otherwise.
#include "cs_common.h"
#include "cs_ddimstep.h"
#include "cs_kernels.h"
#include "cs_latent.h"

namespace cs {

namespace {

constexpr int SL_THREADS = 256;
constexpr size_t SL_LDS_BYTES = 49152;    // the LDS of one workgroup: at least one row of float32, all channels at the latents' sizes
static_assert(LATENT_MAX_WIDTH * sizeof(float) <= SL_LDS_BYTES, "one row of the widest frame must fit");

// the step of W consecutive elements at offset `at` of x's and noise_pred's first halves
template <class T, int W, int PRED>
__device__ __forceinline__ Chunk<T, W> step_chunk(const T* x, const T* __restrict__ noise_pred, size_t at, size_t half, const StepCoeffs& k) {
    const Chunk<T, W> s = load<T, W>(x + at), u = load<T, W>(noise_pred + at), c = load<T, W>(noise_pred + half + at);
    Chunk<T, W> out;
#pragma unroll
    for (int q = 0; q < W; q++) {
        const float e = guided<T>((float)u.v[q], (float)c.v[q], true, k.guidance);
        out.v[q] = (T)ddim_value<T, PRED>((float)s.v[q], e, k);
    }
    return out;
}

}  // namespace

// grid: B * h workgroups, one per (b, row).  group: channels per pass, group * w elements of LDS.  x is read and written (not
// __restrict__): every element of it is read by the one thread that writes it, before it does.
template <class T, int W, int PRED>
__global__ void __launch_bounds__(SL_THREADS) k_standard_step(T* x, const T* __restrict__ noise_pred, const int32_t* __restrict__ src_col,
                                                              uint8_t* mask, const T* __restrict__ noise, int nb, int c, int h, int w,
                                                              int group, int op, StepCoeffs k) {
    using U = typename BitsOf<sizeof(T)>::type;
    extern __shared__ __align__(16) unsigned char sl_lds[];
    T* row_left = reinterpret_cast<T*>(sl_lds);   // [group][w]: the new left values of this row
    const int b = blockIdx.x / h, r = blockIdx.x - b * h, tid = threadIdx.x;
    const size_t plane = (size_t)h * w, view = (size_t)c * plane, half = 2 * (size_t)nb * view;
    const size_t left0 = (size_t)b * view + (size_t)r * w;          // (left view b, channel 0, row r, column 0) of x and noise_pred
    const size_t right0 = left0 + (size_t)nb * view;                // the same of right view b
    const size_t pix0 = ((size_t)b * h + r) * w;                    // of src_col and mask
    const int chunks = w / W;
    for (int g0 = 0; g0 < c; g0 += group) {
        const int gc = min(group, c - g0);
        // phase A: the left view's step; with a shift to come its whole row stays in LDS
        for (int item = tid; item < gc * chunks; item += SL_THREADS) {
            const int g = item / chunks, col = (item - g * chunks) * W;
            const size_t at = left0 + (size_t)(g0 + g) * plane + col;
            const Chunk<T, W> v = step_chunk<T, W, PRED>(x, noise_pred, at, half, k);
            store<T, W>(x + at, v);
            store<T, W>(x + half + at, v);
            if (op != CS_STANDARD_NONE) store<T, W>(row_left + (size_t)g * w + col, v);
        }
        if (op != CS_STANDARD_NONE) __syncthreads();
        // phase B: the right view -- its own step, or the left view's new values gathered from LDS
        for (int item = tid; item < gc * chunks; item += SL_THREADS) {
            const int g = item / chunks, col = (item - g * chunks) * W, ch = g0 + g;
            const size_t at = right0 + (size_t)ch * plane + col;
            Chunk<T, W> v;
            if (op != CS_STANDARD_FIRST) v = step_chunk<T, W, PRED>(x, noise_pred, at, half, k);   // FIRST replaces every element
            if (op != CS_STANDARD_NONE) {
                Chunk<T, W> nz;
                if (noise) nz = load<T, W>(noise + left0 + (size_t)ch * plane + col);
#pragma unroll
                for (int q = 0; q < W; q++) {
                    const size_t pix = pix0 + col + q;
                    const int src = src_col[pix];
                    // (the gather and the mask: cs_latent.h, the statement k_latent_shift_apply uses, here on the LDS row)
                    const bool landed = shift_landed(src, w);
                    const T moved = shift_gathered(landed, row_left, (size_t)g * w + src);
                    bool m;
                    if (op == CS_STANDARD_FIRST && g0 == 0) {
                        const T v0 = shift_gathered(landed, row_left, src);
                        m = shift_mask(__builtin_bit_cast(U, v0));
                        if (g == 0) mask[pix] = m ? 1 : 0;
                    } else {
                        m = mask[pix] != 0;   // RESHIFT: the stored mask; FIRST, a later group: what the first group stored
                    }
                    if (op == CS_STANDARD_FIRST)
                        v.v[q] = (noise && !m) ? nz.v[q] : moved;
                    else if (m)
                        v.v[q] = moved;
                }
            }
            store<T, W>(x + at, v);
            store<T, W>(x + half + at, v);
        }
        if (op != CS_STANDARD_NONE && g0 + group < c) __syncthreads();   // the next group overwrites the LDS rows
    }
}

template <class T, int PRED>
static void standard_step(void* x, const void* noise_pred, const int32_t* src_col, uint8_t* mask, const void* noise, int b, int c, int h,
                          int w, int op, const StepCoeffs& k, hipStream_t stream) {
    constexpr int W = 16 / sizeof(T);
    const size_t row_bytes = (size_t)w * sizeof(T);
    const size_t fit = SL_LDS_BYTES / row_bytes;   // >= 1: w <= LATENT_MAX_WIDTH
    const int group = op == CS_STANDARD_NONE ? c : (int)(fit < (size_t)c ? fit : (size_t)c);
    const size_t lds = op == CS_STANDARD_NONE ? 0 : (size_t)group * row_bytes;
    // whole chunks per row, and every row then starts on the 16-byte grid
    launch_wide_or_narrow(w % W == 0 && aligned16({x, noise_pred, noise}), k_standard_step<T, W, PRED>, k_standard_step<T, 1, PRED>,
                          dim3((unsigned)((size_t)b * h)), dim3(SL_THREADS), lds, stream, as<T>(x), as<T>(noise_pred), src_col, mask,
                          as<T>(noise), b, c, h, w, group, op, k);
}

hipError_t launch_standard_step(void* x, const void* noise_pred, int dtype, int b, int c, int h, int w, float guidance, const float cf[4],
                                int prediction, int op, const int32_t* src_col, uint8_t* mask, const void* noise, hipStream_t stream) {
    const StepCoeffs k{guidance, cf[0], cf[1], cf[2], cf[3]};
    with_latent_type(dtype, [&](auto tag) {
        with_prediction(prediction, [&](auto pred) {
            standard_step<decltype(tag), decltype(pred)::value>(x, noise_pred, src_col, mask, noise, b, c, h, w, op, k, stream);
        });
    });
    return hipGetLastError();
}

}  // namespace cs
