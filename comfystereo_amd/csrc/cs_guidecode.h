// cs_guidecode.h -- the 8-bit code of a guide image's float32 channel, as the passes that read a colour guide take it
// (cs_guideddepth.hip: the colour distance; cs_motiondepth.hip: the luma of the block matcher).  Defined here and nowhere else.
#pragma once
#include "cs_common.h"

namespace cs {

// code(v) = uint8(trunc(min(max(v, 0), 1) * 255 + 0.5)), NaN -> 0 (a NaN fails the first comparison)
__device__ __forceinline__ uint32_t guide_code(float v) {
    float c = v > 0.0f ? v : 0.0f;
    c = c < 1.0f ? c : 1.0f;
    return (uint32_t)(c * 255.0f + 0.5f);
}
__device__ __forceinline__ uint32_t guide_pack(float r, float g, float b) { return guide_code(r) | (guide_code(g) << 8) | (guide_code(b) << 16); }

}  // namespace cs
