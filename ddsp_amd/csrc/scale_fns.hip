// The elementwise functions of ddsp/core.py that csrc/sinusoidal.hip's conversions leave out: the psychoacoustic scales
// (hz_to_bark, bark_to_hz, hz_to_mel, mel_to_hz, hz_to_erb :351-382), soft_limit (:236-238), log_scale (:229-233),
// sym_exp_sigmoid (:407-411) and nan_to_num (:202-204), each with its derivative.  One value per thread, one kernel per
// direction; the constants an op derives from its two parameters are made once on the host, in fp64.
//
// The forward formulas are the reference's own, operation for operation where IEEE arithmetic decides the result at a pole
// (hz_to_bark(0) = -0.53 through 1960 / 0 = inf; bark_to_hz(-0.53) = 0 through 26.81 / 0 = inf).  The derivatives are the
// closed forms without the removable singularities: 26.81 * 1960 / (hz + 1960)^2 is finite at hz = 0.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "launch.h"

namespace ddsp {
namespace scale_fns {

constexpr int kThreads = 256;
constexpr unsigned kMaxBlocks = 1u << 20;
constexpr float kLn10 = 2.302585092994046f;

struct ScaleArgs { float a, b, c; };          // per op, see constants_of

__device__ __forceinline__ float softplus(float z) { return fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float sigmoid(float z) {
  const float e = expf(-fabsf(z)), s = 1.0f / (1.0f + e);        // sigmoid(|z|)
  return z >= 0.0f ? s : e * s;
}

__device__ __forceinline__ float scale_value(int op, float x, ScaleArgs k) {
  switch (op) {
    case DDSP_SCALE_HZ_TO_BARK: return 26.81f / (1.0f + (1960.0f / x)) - 0.53f;
    case DDSP_SCALE_BARK_TO_HZ: return 1960.0f / (26.81f / (x + 0.53f) - 1.0f);
    case DDSP_SCALE_HZ_TO_MEL: {                                  // 2595 logb(1 + hz / 700, 10): safe_log's eps is 1e-5
      const float u = 1.0f + x / 700.0f;
      return 2595.0f * (logf(u <= 0.0f ? 1e-5f : u) / kLn10);
    }
    case DDSP_SCALE_MEL_TO_HZ: return 700.0f * (expf(x * k.a) - 1.0f);              // a = ln 10 / 2595
    case DDSP_SCALE_HZ_TO_ERB: return fmaf(0.108f, x, 24.7f);
    case DDSP_SCALE_SOFT_LIMIT: return (softplus(x) + k.a) - softplus(x - k.b);      // a = x_min, b = x_max - x_min
    case DDSP_SCALE_LOG_SCALE: return k.a * exp2f((0.5f * (x + 1.0f)) * k.b);        // a = min_x, b = log2(max_x / min_x)
    case DDSP_SCALE_SYM_EXP_SIGMOID: {                            // exp_sigmoid(width (|x| / 2 - 1)): a = width
      const float z = k.a * (0.5f * fabsf(x) - 1.0f);
      return fmaf(2.0f, expf(-kLn10 * softplus(-z)), 1e-7f);
    }
    default: return x != x ? k.a : x;                             // DDSP_SCALE_NAN_TO_NUM: a = value
  }
}

__device__ __forceinline__ float scale_slope(int op, float x, ScaleArgs k) {
  switch (op) {
    case DDSP_SCALE_HZ_TO_BARK: { const float d = x + 1960.0f; return (26.81f * 1960.0f) / (d * d); }
    case DDSP_SCALE_BARK_TO_HZ: { const float d = 26.81f - (x + 0.53f); return (26.81f * 1960.0f) / (d * d); }
    case DDSP_SCALE_HZ_TO_MEL: return (1.0f + x / 700.0f) <= 0.0f ? 0.0f : (2595.0f / kLn10) / (700.0f + x);
    case DDSP_SCALE_MEL_TO_HZ: return (700.0f * k.a) * expf(x * k.a);
    case DDSP_SCALE_HZ_TO_ERB: return 0.108f;
    case DDSP_SCALE_SOFT_LIMIT: return sigmoid(x) - sigmoid(x - k.b);
    case DDSP_SCALE_LOG_SCALE: return (k.a * exp2f((0.5f * (x + 1.0f)) * k.b)) * k.c;   // c = ln(max_x / min_x) / 2
    case DDSP_SCALE_SYM_EXP_SIGMOID: {
      const float z = k.a * (0.5f * fabsf(x) - 1.0f);
      const float body = 2.0f * expf(-kLn10 * softplus(-z));                        // 2 sigmoid(z)^ln 10
      const float sign = x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f);               // tf.abs: slope 0 at 0
      return body * kLn10 * sigmoid(-z) * (0.5f * k.a) * sign;
    }
    default: return x != x ? 0.0f : 1.0f;
  }
}

template <bool BWD>
__global__ __launch_bounds__(kThreads) void scale_convert_kernel(const float* __restrict__ in, const float* __restrict__ grad_out,
                                                                 float* __restrict__ out, size_t n, int op, ScaleArgs k) {
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
    const float x = in[i];
    if (BWD) {
      const float slope = scale_slope(op, x, k);
      out[i] = (op == DDSP_SCALE_NAN_TO_NUM && slope == 0.0f) ? 0.0f : grad_out[i] * slope;
    } else {
      out[i] = scale_value(op, x, k);
    }
  }
}

static bool constants_of(int op, float p0, float p1, ScaleArgs& k) {
  k = ScaleArgs{0.0f, 0.0f, 0.0f};
  switch (op) {
    case DDSP_SCALE_HZ_TO_BARK: case DDSP_SCALE_BARK_TO_HZ: case DDSP_SCALE_HZ_TO_MEL: case DDSP_SCALE_HZ_TO_ERB: return true;
    case DDSP_SCALE_MEL_TO_HZ: k.a = (float)(log(10.0) / 2595.0); return true;
    case DDSP_SCALE_SOFT_LIMIT: k.a = p0; k.b = (float)((double)p1 - (double)p0); return true;
    case DDSP_SCALE_LOG_SCALE: {
      const double ratio = (double)p1 / (double)p0;
      k.a = p0; k.b = (float)log2(ratio); k.c = (float)(0.5 * log(ratio));
      return true;
    }
    case DDSP_SCALE_SYM_EXP_SIGMOID: case DDSP_SCALE_NAN_TO_NUM: k.a = p0; return true;
    default: return false;
  }
}

static unsigned blocks_for(size_t n) {
  const size_t g = (n + kThreads - 1) / kThreads;
  return (unsigned)(g > kMaxBlocks ? kMaxBlocks : g);
}

}  // namespace scale_fns
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::scale_fns;

extern "C" int ddsp_scale_convert_f32(const float* in, float* out, size_t n, int op, float p0, float p1, void* stream) {
  if (!in || !out) return DDSP_ERR_NULL_POINTER;
  ScaleArgs k;
  if (!constants_of(op, p0, p1, k)) return DDSP_ERR_BAD_SHAPE;
  if (n == 0) return DDSP_OK;
  hipLaunchKernelGGL(scale_convert_kernel<false>, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, in,
                     (const float*)nullptr, out, n, op, k);
  return check_launch();
}

extern "C" int ddsp_scale_convert_backward_f32(const float* in, const float* grad_out, float* grad_in, size_t n, int op, float p0,
                                               float p1, void* stream) {
  if (!in || !grad_out || !grad_in) return DDSP_ERR_NULL_POINTER;
  ScaleArgs k;
  if (!constants_of(op, p0, p1, k)) return DDSP_ERR_BAD_SHAPE;
  if (n == 0) return DDSP_OK;
  hipLaunchKernelGGL(scale_convert_kernel<true>, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, in, grad_out, grad_in,
                     n, op, k);
  return check_launch();
}
