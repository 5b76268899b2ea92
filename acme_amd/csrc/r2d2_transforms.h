// R2D2's value transforms (acme/tf/losses/r2d2.py:172-180) and the correctly rounded f32
// helpers they need, in TF's f32 operation order with no contraction.  One definition for the
// two loss kernels that must give the same bits: r2d2_learner.hip (r2d2_loss_kernel) and
// r2d2_mlp.hip (the loss inside r2d2_mlp_unroll_kernel).
//
// ACME_R2D2_TX_ATTR: extra function attributes, set by a translation unit whose kernels carry
// target features of their own (functions with other target features do not inline).
#pragma once

#include <hip/hip_runtime.h>

#ifndef ACME_R2D2_TX_ATTR
#define ACME_R2D2_TX_ATTR
#endif
#define ACME_R2D2_TX __device__ __forceinline__ ACME_R2D2_TX_ATTR

namespace acme {

ACME_R2D2_TX float sgnf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : x); }

// IEEE (correctly rounded) f32 square root and quotient: evaluated in f64 and rounded once
// to f32, which is exact for both (53 >= 2 x 24 + 2 bits: the double rounding is innocuous).
// (__fsqrt_rn without OCML_BASIC_ROUNDED_OPERATIONS is the native approximation.)
ACME_R2D2_TX float sqrt_rn(float x) { return (float)__builtin_sqrt((double)x); }
ACME_R2D2_TX float div_rn(float x, float y) { return (float)((double)x / (double)y); }

// _signed_hyperbolic_tx (losses/r2d2.py:172-174): sign(x) (sqrt(|x| + 1) - 1) + eps x, in
// TF's f32 operation order, no contraction.
ACME_R2D2_TX float hyperbolic(float x) {
#pragma clang fp contract(off)
  const float s = sqrt_rn(fabsf(x) + 1.f) - 1.f;
  return sgnf(x) * s + 1e-3f * x;
}

// _signed_parabolic_tx (:177-180): z = sqrt(1 + 4 eps (eps + 1 + |x|)) / 2 / eps - 1 / 2 / eps
// (Python folds eps + 1 and 4 eps and 1 / 2 / eps into f32 constants); sign(x) (z^2 - 1).
ACME_R2D2_TX float parabolic(float x) {
#pragma clang fp contract(off)
  const float t = 0.004f * (1.001f + fabsf(x));
  const float z = div_rn(sqrt_rn(1.f + t) * 0.5f, 1e-3f) - 500.f;  // x / 2 exact as x * 0.5
  return sgnf(x) * (z * z - 1.f);
}

}  // namespace acme
