// cs_attention_half.h -- what the half-input MFMA kernels of cs_attention_half.hip (forward) and cs_attention_half_bwd.hip
// (backward) share: the fragment types of v_mfma_f32_32x32x16_f16 / _bf16, the accumulator's row map, and the slot order of the
// transposed, row-permuted LDS images that make registers 8 s .. 8 s + 7 of an accumulator the B fragment of k-step s.
#pragma once
#include "cs_common.h"

namespace cs {

enum { SAH_KT = 32, SAH_SVT = SAH_KT + 8 };   // rows per tile; halves per row of a transposed image (80 bytes)

typedef float sah_acc __attribute__((ext_vector_type(16)));
typedef _Float16 sah_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sah_bf16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct sah_frag;
template <> struct sah_frag<_Float16> {
    typedef sah_f16x8 type;
    static __device__ __forceinline__ sah_acc mfma(type a, type b, sah_acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct sah_frag<__bf16> {
    typedef sah_bf16x8 type;
    static __device__ __forceinline__ sah_acc mfma(type a, type b, sah_acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

// accumulator register r of lane half hi <-> row of the 32 x 32 tile (cs_attention.hip sa_row)
__device__ __forceinline__ int sah_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
// row of a tile -> its position in a row of a transposed image: the inverse of sah_row(8 s + j, h) -> 16 s + 8 h + j
__device__ __forceinline__ int sah_slot(int key) { return (key & 16) + 8 * ((key >> 2) & 1) + 4 * ((key >> 3) & 1) + (key & 3); }

// half element i (0..7) of a 16-byte chunk
__device__ __forceinline__ unsigned sah_elem(const uint4& c, int i) {
    const unsigned w = (i >> 1) == 0 ? c.x : (i >> 1) == 1 ? c.y : (i >> 1) == 2 ? c.z : c.w;
    return (i & 1) ? (w >> 16) : (w & 0xffffu);
}

}  // namespace cs
