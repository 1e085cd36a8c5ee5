// Device helpers shared by the kernels that own one frame of sinusoids per block (consistency.hip, wasserstein.hip): the
// block's geometry, hz_to_midi as an fp32 pair and the fixed-order block sum.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace ddsp {
namespace consistency {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr float kMidiSlope = 17.312340490667562f;      // 12 / ln 2: d hz_to_midi(f) / df = kMidiSlope / f

// core.hz_to_midi: 12 (log2 f - log2 440) + 69, f <= 0 -> 0.  Taken in fp64 and kept as an fp32 pair hi + lo: a Gaussian's
// exponent is ((x - mu) / s)^2 / 2 with s down to 0.02 MIDI, and an ulp of a MIDI value near 100 is 7.6e-6 - the difference
// of two values rounded to fp32 would carry that into the exponent (at 20 MIDI apart and s = 0.1: 1e-6 of the loss, ten
// times the reference's own error).  (x_hi - mu_hi) + (x_lo - mu_lo) is good to an ulp of the DIFFERENCE.  One fp64 log2 per
// frame and value, two more fp32 additions per term.
__device__ __forceinline__ float hz_to_midi(float hz, float& lo) {
  if (hz <= 0.0f) { lo = 0.0f; return 0.0f; }
  const double m = 12.0 * (log2((double)hz) - 8.78135971352466) + 69.0;
  const float hi = (float)m;
  lo = (float)(m - (double)hi);
  return hi;
}
__device__ __forceinline__ float hz_to_midi(float hz) { float lo; return hz_to_midi(hz, lo); }

// sum over the block in a fixed order; every thread receives it.  red: kWaves doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace consistency
}  // namespace ddsp
