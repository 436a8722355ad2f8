// cs_latent.h -- what the kernels of the latent loops share besides their arithmetic (cs_ddimstep.h): the 16-byte access, the
// shift's gather and hole test, and on the host the dtype dispatch and the choice between a kernel's wide and its narrow form.
// cs_latentshift.hip, cs_inversion.hip, cs_inpaintloop.hip and cs_standardloop.hip launch through it; cs_abi.hip takes the
// element size and the width limit from it.  One definition of each: a copy in a translation unit is a bug waiting for a fix
// that reaches only one of them.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "cs_common.h"

namespace cs {

// cs_latent_shift_plan's limit on a row, which cs_standard_step inherits: the tables come from there.  The plan's destination
// table of a row stays within 32 KiB of LDS, one float32 row of the step within its 48 KiB.
constexpr int LATENT_MAX_WIDTH = 8192;

inline size_t latent_elem_bytes(int dtype) { return dtype == CS_LATENT_F32 ? 4 : 2; }

// ---- device: access ------------------------------------------------------------------------------------------------------------
// W consecutive elements of T moved as one access (W * sizeof(T) bytes, a power of two; 16 at the most per instruction)
template <class T, int W>
struct alignas((W * sizeof(T) >= 16) ? 16 : W * sizeof(T)) Chunk {
    T v[W];
};
template <class T, int W>
__device__ __forceinline__ Chunk<T, W> load(const T* p) { return *reinterpret_cast<const Chunk<T, W>*>(p); }
template <class T, int W>
__device__ __forceinline__ void store(T* p, const Chunk<T, W>& c) { *reinterpret_cast<Chunk<T, W>*>(p) = c; }

// an element as the unsigned integer of its size: the shift moves values and never computes
template <int BYTES> struct BitsOf;
template <> struct BitsOf<4> { using type = uint32_t; };
template <> struct BitsOf<2> { using type = uint16_t; };

// ---- device: the latent shift (reference stereodiffusion_nodes.py:650-667) -------------------------------------------------------
// A destination column takes the left view's value at column src of its row, where one landed: src_col holds -1 in a hole.
__device__ __forceinline__ bool shift_landed(int src, int w) { return (unsigned)src < (unsigned)w; }

// the gathered value: view[at] -- the left view at the source column, in global memory for k_latent_shift_apply, in the LDS row for
// k_standard_step; not read where nothing landed -- or 0
template <class V>
__device__ __forceinline__ V shift_gathered(bool landed, const V* view, size_t at) {
    return landed ? view[at] : (V)0;
}

// The mask of a pixel, `channel 0 of the gathered view != 0`, on the value's bits: some bit but the sign is set.  +-0.0 is a hole,
// a NaN is not.
template <class U>
__device__ __forceinline__ bool shift_mask(U bits) {
    const U abs_bits = (U)~((U)1 << (8 * sizeof(U) - 1));
    return (bits & abs_bits) != 0;
}

// ---- host: launch plumbing -----------------------------------------------------------------------------------------------------
inline bool aligned16(std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    return (bits & 15) == 0;
}

// the grid of a grid-stride kernel of 256 threads over `items`
inline int stream_grid(size_t items) {
    const size_t blocks = (items + 255) / 256;
    return (int)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

// f(T{}) with T the element type of `dtype` (enum cs_latent_dtype, checked by the caller): with_latent_type(dtype, [&](auto tag) {
// using T = decltype(tag); ... })
template <class F>
void with_latent_type(int dtype, F&& f) {
    if (dtype == CS_LATENT_F32)
        f(float{});
    else if (dtype == CS_LATENT_F16)
        f(_Float16{});
    else
        f(__bf16{});
}

// f(tag) with decltype(tag)::value the prediction type (enum cs_prediction, checked by the caller), a compile-time constant:
// with_prediction(prediction, [&](auto pred) { constexpr int P = decltype(pred)::value; ... })
template <class F>
void with_prediction(int prediction, F&& f) {
    if (prediction == CS_PRED_V)
        f(std::integral_constant<int, CS_PRED_V>{});
    else
        f(std::integral_constant<int, CS_PRED_EPSILON>{});
}

// a void* argument as the kernel's element pointer
template <class T> const T* as(const void* p) { return static_cast<const T*>(p); }
template <class T> T* as(void* p) { return static_cast<T*>(p); }

// one kernel in two instantiations of one signature: the 16-byte form where `wide` holds, one element per access otherwise
template <class... Params, class... Args>
void launch_wide_or_narrow(bool wide, void (*k_wide)(Params...), void (*k_narrow)(Params...), dim3 grid, dim3 block, size_t lds,
                           hipStream_t stream, Args... args) {
    hipLaunchKernelGGL(wide ? k_wide : k_narrow, grid, block, lds, stream, static_cast<Params>(args)...);
}

}  // namespace cs
