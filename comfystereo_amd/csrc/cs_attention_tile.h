// cs_attention_tile.h -- what the four attention translation units share: cs_attention.hip / cs_attention_bwd.hip (float32, on
// v_mfma_f32_32x32x2_f32) and cs_attention_half.hip / cs_attention_half_bwd.hip (float16 / bfloat16, on v_mfma_f32_32x32x16_f16 /
// _bf16).  Device side: the 32 x 32 tile's edge, accumulator type and row map, the half fragments and their transposed LDS images.
// Host side: the one map from (head dimension, waves per workgroup) to a kernel instantiation, and the half dtype selector.
// The per-tile arithmetic (online softmax, P / dS, the epilogue's row store) is spelled out in each kernel: as shared
// __forceinline__ helpers it gave the same bits but other register assignments and schedules, and measured slower (docs/HISTORY.md).
//
// The accumulator.  All kernels compute 32 x 32 tiles whose COLUMN is on the lane (l & 31) and whose 16 rows per lane half
// hi = l >> 5 are in the registers: register r is row at_row(r, hi) = (r & 3) + 8 (r >> 2) + 4 hi.  With the query on the lane (the
// forwards, the dq kernels) softmax's row reductions are in-lane plus one exchange with lane l ^ 32; after the last tile lane
// (column, hi) holds output columns 32 b + 8 g + 4 hi .. + 3 of its row in registers 4 g .. 4 g + 3 of block b.
//
// The half fragments.  Lane (r, h) (r = l & 31, h = l >> 5) of an A fragment holds row r, k = 8 h + j (j = 0..7): one ds_read_b128
// from a row-major image.  Registers 8 s .. 8 s + 7 of an accumulator, converted to half, ARE the B fragment of k-step s (s = 0, 1)
// of the next product: element j stands for row at_row(8 s + j, h) = 16 s + 8 (j >> 2) + 4 h + (j & 3).  The A fragment of that
// product is the other operand of those eight rows at column 32 b + r, so that operand is staged TRANSPOSED and row-permuted,
// img[column][slot 16 s + 8 h + j] (sah_slot), rows SAH_SVT halves apart, and the fragment is again one ds_read_b128.
// LDS banking (16-byte slots, 16 per 256-byte bank row; ds_read_b128 is served in 16-lane groups {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} of either wave half, i.e. one h and 16 rows that are pairwise distinct mod 16):
//   rows of a row-major image are 32 ND + 8 halves = (4 ND + 1) slots apart, rows of a transposed one 40 halves = 5 slots: an odd
//   slot stride times 16 rows distinct mod 16 gives 16 distinct slots, every fragment read is conflict-free.
//   The transposing store (sah_store_t; the half forward spells it out in stage()) is a ds_write_b32 of the row pair (2 m, 2 m + 1) -- adjacent slots -- per column: a wave
//   half is 16 pairs x two 8-column chunks; the 16 pairs fill 16 consecutive dwords of an image row, rows are 20 dwords apart, 8 rows
//   are 160 = 0 (mod 32) dwords apart, so the lanes of the odd chunk take their columns in the order i ^ 4 (4 rows = 80 = 16 mod 32):
//   the two chunks land on disjoint halves of the 32 write banks.
#pragma once
#include <type_traits>

#include "cs_common.h"

namespace cs {

enum { AT_T = 32, SAH_SVT = AT_T + 8 };   // rows (keys or queries) per tile; halves per row of a transposed image (80 bytes)

typedef float at_acc __attribute__((ext_vector_type(16)));
typedef _Float16 sah_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sah_bf16x8 __attribute__((ext_vector_type(8)));

template <typename T> struct sah_frag;
template <> struct sah_frag<_Float16> {
    typedef sah_f16x8 type;
    static __device__ __forceinline__ at_acc mfma(type a, type b, at_acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct sah_frag<__bf16> {
    typedef sah_bf16x8 type;
    static __device__ __forceinline__ at_acc mfma(type a, type b, at_acc c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

// accumulator register r of lane half hi <-> row of the 32 x 32 tile
__device__ __forceinline__ int at_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
// row of a tile -> its position in a row of a transposed image: the inverse of at_row(8 s + j, h) -> 16 s + 8 h + j
__device__ __forceinline__ int sah_slot(int key) { return (key & 16) + 8 * ((key >> 2) & 1) + 4 * ((key >> 3) & 1) + (key & 3); }

// half element i (0..7) of a 16-byte chunk
__device__ __forceinline__ unsigned sah_elem(const uint4& c, int i) {
    const unsigned w = (i >> 1) == 0 ? c.x : (i >> 1) == 1 ? c.y : (i >> 1) == 2 ? c.z : c.w;
    return (i & 1) ? (w >> 16) : (w & 0xffffu);
}

// Stores columns 8 c8 .. 8 c8 + 7 of the row pair (2 m, 2 m + 1) -- lo and up -- into a transposed image at `slot` = sah_slot(2 m):
// eight ds_write_b32, the odd chunks in the order i ^ 4 (the banking argument above).
template <typename T>
__device__ __forceinline__ void sah_store_t(T* img, const uint4& lo, const uint4& up, int c8, int slot) {
    const bool odd = c8 & 1;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int ii = odd ? (i ^ 4) : i;
        *(unsigned*)(img + (8 * c8 + ii) * SAH_SVT + slot) = sah_elem(lo, ii) | (sah_elem(up, ii) << 16);
    }
}

// Host: maps (d, nw) to compile-time (ND = head-dim blocks of 32, NW = waves per workgroup) and calls
// f(std::integral_constant<int, ND>, std::integral_constant<int, NW>); hipErrorInvalidValue for ND outside 1..5.
template <typename F>
static hipError_t at_dispatch(int d, int nw, F f) {
    auto waves = [&](auto nd) {
        if (nw == 4) return f(nd, std::integral_constant<int, 4>());
        if (nw == 2) return f(nd, std::integral_constant<int, 2>());
        return f(nd, std::integral_constant<int, 1>());
    };
    switch ((d + 31) / 32) {
    case 1: return waves(std::integral_constant<int, 1>());
    case 2: return waves(std::integral_constant<int, 2>());
    case 3: return waves(std::integral_constant<int, 3>());
    case 4: return waves(std::integral_constant<int, 4>());
    case 5: return waves(std::integral_constant<int, 5>());
    }
    return hipErrorInvalidValue;
}

// Host: the half kernels' element type from enum cs_attn_dtype: calls f with a null T* as the type's tag.
template <typename F>
static hipError_t sah_dispatch(int dtype, F f) {
    if (dtype == CS_ATTN_F16) return f((_Float16*)nullptr);
    if (dtype == CS_ATTN_BF16) return f((__bf16*)nullptr);
    return hipErrorInvalidValue;
}

}  // namespace cs
