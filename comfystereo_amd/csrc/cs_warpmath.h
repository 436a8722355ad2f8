// cs_warpmath.h -- the float32 steps forward_warp_gpu and the grid-sample warps of the reference share (depth -> offset curve,
// torch.linspace(-1, 1, n), grid_sample's unnormalisation), used by cs_gpuwarp.hip and cs_gridwarp.hip.
#pragma once
#include "cs_math.h"

namespace cs {

// torch.pow(x, e) with a scalar exponent, by the exponent class pow_mode_of() picked on the host: torch special-cases
// 1 (copy), 0.5 (sqrt), 2 (x * x), 3 ((x * x) * x) and 0 (ones); every other exponent is libm's powf
__device__ __forceinline__ float torch_pow(float x, int mode, float e32, const csm::PowfTables* T) {
    switch (mode) {
    case 0: return x;
    case 1: return sqrtf(x);
    case 2: return x * x;
    case 3: return (x * x) * x;
    case 5: return 1.0f;
    default: return csm::powf_exact(x, e32, T);
    }
}
static inline int pow_mode_of(double e) { return e == 1.0 ? 0 : e == 0.5 ? 1 : e == 2.0 ? 2 : e == 3.0 ? 3 : e == 0.0 ? 5 : 4; }

// torch.linspace(-1, 1, n)[i] for n >= 2, step = 2 / (n - 1) (an IEEE float32 division): CPU torch fills the two halves from
// either end, each value one fused multiply-add (bit-equal to CPU torch for every n up to 16 384; n == 1 gives [-1])
__device__ __forceinline__ float torch_linspace_m11(int i, int n, float step) {
    return i < n / 2 ? fmaf(step, (float)i, -1.0f) : fmaf(-step, (float)(n - i - 1), 1.0f);
}

// grid_sample's unnormalisation with align_corners=True: [-1, 1] -> [0, size - 1]
__device__ __forceinline__ float gs_unnormalize(float g, int size) { return (g + 1.0f) * ((float)(size - 1) / 2.0f); }

}  // namespace cs
