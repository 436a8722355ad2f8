// cs_gridsample.h -- device pieces the grid-sample kernels share (cs_gridwarp.hip, cs_inpaintprep.hip): CPU torch's grid_sample
// (align_corners=True) as it runs -- the four corner taps summed as fma(se, fma(sw, fma(ne, nw * v0))), the reflection remainder
// one fused multiply-add -- and the bit rows of a masked image row with their "nearest valid column" searches.
#pragma once
#include "cs_common.h"
#include "cs_warpmath.h"

namespace cs {

// grid_sample's source coordinate on one axis (align_corners=True) under a padding mode
__device__ __forceinline__ float gs_coord(float g, int size, int padding) {
    float x = gs_unnormalize(g, size);
    if (padding == CS_GRID_PAD_REFLECTION) {
        if (size <= 1) {
            x = 0.0f;
        } else {
            const float span = (float)(size - 1) * 2.0f;
            const float a = fabsf(x);
            const float flips = truncf(a / span);
            const float extra = __builtin_fmaf(-flips, span, a);
            x = fminf(extra, span - extra);
        }
    }
    if (padding != CS_GRID_PAD_ZEROS) x = fminf(fmaxf(x, 0.0f), (float)(size - 1));
    return x;
}

// the vertical half of a bilinear tap set: rows, weights and whether each row is read (zeros padding: rows outside are 0)
struct RowTaps { int y0, y1; float n, s; bool in0, in1; };
__device__ __forceinline__ RowTaps row_taps(float gy, int h, int padding) {
    const float yc = gs_coord(gy, h, padding);
    const float yn = floorf(yc);
    RowTaps R;
    R.n = yc - yn;
    R.s = 1.0f - R.n;
    const float y1 = yn + 1.0f;
    R.in0 = padding != CS_GRID_PAD_ZEROS || (yn > -1.0f && yn < (float)h);
    R.in1 = padding != CS_GRID_PAD_ZEROS ? y1 < (float)h : (y1 > -1.0f && y1 < (float)h);
    R.y0 = R.in0 ? (int)yn : 0;
    R.y1 = R.in1 ? (int)y1 : 0;
    return R;
}

// the C channels of one output pixel: bilinear at grid x `g` on the rows R of image plane `img` ([c][h][w])
// (out[ch * ostride]: the output's channel stride, the image's is `plane`)
__device__ __forceinline__ void sample_pixel_strided(const float* img, float* out, size_t ostride, int c, int h, int w, size_t plane,
                                                     float g, const RowTaps& R, int padding) {
    const float xc = gs_coord(g, w, padding);
    const float xw = floorf(xc);
    const float wt = xc - xw, et = 1.0f - wt;
    const float nw = R.s * et, ne = R.s * wt, sw = R.n * et, se = R.n * wt;
    const float x1 = xw + 1.0f;
    const bool inw = padding != CS_GRID_PAD_ZEROS || (xw > -1.0f && xw < (float)w);
    const bool ine = padding != CS_GRID_PAD_ZEROS ? x1 < (float)w : (x1 > -1.0f && x1 < (float)w);
    const int ix0 = inw ? (int)xw : 0, ix1 = ine ? (int)x1 : 0;
    const bool a = R.in0 && inw, b = R.in0 && ine, cc = R.in1 && inw, d = R.in1 && ine;
    const float* r0 = img + (size_t)R.y0 * w;
    const float* r1 = img + (size_t)R.y1 * w;
    for (int ch = 0; ch < c; ch++) {
        const float v0 = a ? r0[ix0] : 0.0f, v1 = b ? r0[ix1] : 0.0f, v2 = cc ? r1[ix0] : 0.0f, v3 = d ? r1[ix1] : 0.0f;
        out[(size_t)ch * ostride] = __builtin_fmaf(v3, se, __builtin_fmaf(v2, sw, __builtin_fmaf(v1, ne, v0 * nw)));
        r0 += plane; r1 += plane;
    }
}
__device__ __forceinline__ void sample_pixel(const float* img, float* out, int c, int h, int w, size_t plane, float g,
                                             const RowTaps& R, int padding) {
    sample_pixel_strided(img, out, plane, c, h, w, plane, g, R, padding);
}

// inclusive prefix maximum over the 64 lanes of a wave
__device__ __forceinline__ int wave_prefix_max(int v) {
    const int lane = lane_id();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off);
        if (lane >= off) v = max(v, u);
    }
    return v;
}

// validity bits of word `wi` of a row: the columns that exist and are not gaps
__device__ __forceinline__ uint32_t valid_word(const uint32_t* gapb, int wi, int w) {
    const int rem = w - 32 * wi;
    const uint32_t in = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
    return ~gapb[wi] & in;
}

// "left border" of column x: the highest valid column below x (-1: none), from the row's bits and word maxima
__device__ __forceinline__ int left_valid(const uint32_t* gapb, const int* last, int x, int w) {
    const int wi = x >> 5, b = x & 31;
    const uint32_t below = valid_word(gapb, wi, w) & ((1u << b) - 1u);
    if (below) return wi * 32 + 31 - __clz((int)below);
    return wi > 0 ? last[wi - 1] : -1;
}

// last[wi] = the highest valid column in words 0..wi (-1: none); the block's `last valid column` is the return value.
// Called by every thread of the block (contains barriers); gapb must be complete.
__device__ int word_prefix_last(const uint32_t* gapb, int* last, int* red, int w) {
    const int nwords = (w + 31) >> 5, tid = threadIdx.x;
    if (tid < 64) {
        int carry = -1;
        for (int base = 0; base < nwords; base += 64) {
            const int wi = base + tid;
            int v = -1;
            if (wi < nwords) {
                const uint32_t m = valid_word(gapb, wi, w);
                v = m ? wi * 32 + 31 - __clz((int)m) : -1;
            }
            v = max(wave_prefix_max(v), carry);
            if (wi < nwords) last[wi] = v;
            carry = __shfl(v, 63);
        }
        if (tid == 0) red[0] = carry;
    }
    __syncthreads();
    return red[0];
}

}  // namespace cs
