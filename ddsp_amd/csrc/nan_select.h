// ReLU, max and min that KEEP a NaN operand, as tf.nn.relu, tf.maximum, tf.minimum and tf.clip_by_value do (and torch's):
// fmaxf / fminf return the other operand, and `u > 0 ? u : 0` returns the 0 - either way a NaN that the reference would hand on to
// the loss vanishes inside the kernel, and a diverged decoder trains on as if nothing had happened ("Non-finite
// values", R3).  One compare and one select each, the cost of the forms they replace; for every other operand the result is
// fmaxf's / fminf's (a -0 against a +0 bound gives the +0 bound).  Where a maximum clamps an INDEX, fmaxf's dropping of the NaN
// is what keeps the index in range: those sites keep fmaxf (the audit table).
#pragma once
#include <hip/hip_runtime.h>

namespace ddsp {

__device__ __forceinline__ float relu_keep_nan(float v) { return v <= 0.0f ? 0.0f : v; }
// `bound` is a constant of the call, never a NaN
__device__ __forceinline__ float max_keep_nan(float v, float bound) { return v <= bound ? bound : v; }
__device__ __forceinline__ float min_keep_nan(float v, float bound) { return v >= bound ? bound : v; }

}  // namespace ddsp
