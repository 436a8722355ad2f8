// cs_ddimstep.h -- the arithmetic of one guided DDIM step, the one statement of it: cs_inversion.hip (k_ddim_step,
// k_null_loss_grad) and cs_standardloop.hip (k_standard_step) include it, so the fused Standard-mode step cannot drift from
// cs_ddim_step, which the fixtures pin.
//
// Every operation of the reference's tensor expression is one operation here, rounded once to the tensors' dtype before the
// next -- float32: plain IEEE (the library is built with -ffp-contract=off); float16 / bfloat16: the operation in float32, then
// the conversion, which is what torch does with a half tensor and a scalar.
#pragma once
#include "cs_common.h"

namespace cs {

// x rounded to T, as a float (float: x itself)
template <class T>
__device__ __forceinline__ float rnd(float x) { return (float)(T)x; }
template <>
__device__ __forceinline__ float rnd<float>(float x) { return x; }

// a * b rounded to T as CPU torch rounds it: the product rounded to float32, that rounded to T.  Left alone, the compiler folds a
// lone float16 product and its conversion into v_fma_mixlo_f16 a, b, +0 -- one rounding of the exact product, and a product of
// -0.0 made positive by the addend -- and packs neighbouring ones into v_pk_mul_f32 with a conversion afterwards, which is the
// other result: what the bits are would depend on how a kernel is unrolled.  The empty asm makes the float32 product a value of
// its own in every kernel: a v_mul_f32, then a v_cvt_f16_f32.  cs_inpaintloop.hip uses this one too.
template <class T>
__device__ __forceinline__ float mul_rnd(float a, float b) {
    float p = a * b;
    asm("" : "+v"(p));
    return rnd<T>(p);
}

struct StepCoeffs {
    float guidance, c1, c2, c3, c4;
};

// e = eps_a + guidance * (eps_b - eps_a) (reference inversion.py:88), or eps_a
template <class T>
__device__ __forceinline__ float guided(float a, float b, bool has_b, float guidance) {
    if (!has_b) return a;
    const float d = rnd<T>(b - a);
    const float gd = mul_rnd<T>(guidance, d);
    return rnd<T>(a + gd);
}

// The step from the guided prediction e, by what the model predicts (PRED: enum cs_prediction; a template parameter, so the
// epsilon instantiations are the code they were):
//   CS_PRED_EPSILON  c4 * ((sample - c1 * e) / c2) + c3 * e, in the reference's order (inversion.py:62-64, :72-74)
//   CS_PRED_V        e is v = c2 * eps - c1 * x0 (Salimans & Ho 2022):  x0 = c2 * sample - c1 * v;  eps = c2 * v + c1 * sample;
//                    c4 * x0 + c3 * eps -- the operation order of diffusers' DDIMScheduler.step with prediction_type
//                    "v_prediction", eta 0.  c2 is the first operand of two products here and divides nothing.
template <class T, int PRED = CS_PRED_EPSILON>
__device__ __forceinline__ float ddim_value(float s, float e, const StepCoeffs& k) {
    if constexpr (PRED == CS_PRED_V) {
        const float x0 = rnd<T>(mul_rnd<T>(k.c2, s) - mul_rnd<T>(k.c1, e));
        const float eps = rnd<T>(mul_rnd<T>(k.c2, e) + mul_rnd<T>(k.c1, s));
        return rnd<T>(mul_rnd<T>(k.c4, x0) + mul_rnd<T>(k.c3, eps));
    }
    const float t = mul_rnd<T>(k.c1, e);
    const float num = rnd<T>(s - t);
    const float x0 = rnd<T>(num / k.c2);
    const float dir = mul_rnd<T>(k.c3, e);
    const float scaled = mul_rnd<T>(k.c4, x0);
    return rnd<T>(scaled + dir);
}

// the same from the prediction before its roundings to T, in float64: what the null-text loss is taken from (cs_nullloss.h)
template <int PRED>
__device__ __forceinline__ double ddim_value_f64(double s, double e, const StepCoeffs& k) {
    if constexpr (PRED == CS_PRED_V) {
        const double x0 = (double)k.c2 * s - (double)k.c1 * e;
        const double eps = (double)k.c2 * e + (double)k.c1 * s;
        return (double)k.c4 * x0 + (double)k.c3 * eps;
    }
    return (double)k.c4 * ((s - (double)k.c1 * e) / (double)k.c2) + (double)k.c3 * e;
}

}  // namespace cs
