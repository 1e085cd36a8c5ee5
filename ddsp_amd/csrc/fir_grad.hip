// The adjoint of the time-varying FIR (core.fft_convolve, ddsp/core.py:1382-1473 with crop_and_compensate_delay :1338-1379),
// the sinc filter design (core.sinc_impulse_response, :1568-1625) forward and backward, the adjoint of the frequency-sampling
// design (core.frequency_impulse_response, :1534-1565) and of core.exp_sigmoid (:386-404), for gfx950.
//
// Forward (general.hip / filtered_noise*.hip):  z[m] = sum_i audio[i] ir[frame(i)][m - i], out[n] = z[n + start], n < n_out,
// frame(i) = i / frame_size, frame_size = ceil(N / F).  With g = dL/d out (terms whose g index leaves [0, n_out) drop):
//
//   dL/d audio[b][i]  = sum_k ir[b or 0][frame(i)][k] g[b][i + k - start]          fir_grad_audio_kernel / _any_kernel
//   dL/d ir[b][f][k]  = sum_{i in frame f} audio[b][i] g[b][i + k - start]         fir_grad_ir_kernel
//
// Both run on the vector ALUs from LDS tiles (the choice DESIGN.md section 4 records): per multiply-add one tap / sample that
// is the same address in (most of) a wavefront and one g value at consecutive addresses - two LDS reads per FMA, which is
// what bounds them.  Nothing is accumulated across threads: every output element is owned by one thread which adds its terms
// in ascending k (audio) or ascending i (ir), so the bits are the same on every call and a row alone equals its row in a batch.
//
//   fir_grad_audio_kernel   a block owns kTile consecutive samples of one row: the taps of the frames the tile touches and
//                           kTile + L - 1 values of g sit in LDS.  Shapes whose taps do not fit (filters on frames so short
//                           that a tile touches too many of them) take fir_grad_audio_any_kernel: one thread per sample,
//                           operands from L2, the same sums in the same order.
//   fir_grad_ir_kernel      a block owns 256 taps of one (row, frame) and walks the frame in chunks of kChunk samples: the
//                           chunk of audio and its chunk + 255 values of g in LDS.  Any shape.
//   A broadcast impulse response (Bir == 1) gets per-row partials [B, F, L] from the same kernel; the host layer adds the
//   rows in a fixed order with ddsp_sum_rows_f32.
//
//   sinc_ir_kernel / sinc_ir_backward_kernel   a block per (row, frame).  The normalising sum, and the four sums of the
//                           backward pass, are per-thread strided partials in fp64 added by thread 0 in thread order.
//   fir_design_backward_kernel   grad_magnitudes[r][m] = sum_k D[k][m] grad_ir[r][k]: the design is linear in the magnitudes,
//                           D [L, M] is what the forward design kernel makes of the identity (the host layer keeps it).
//   exp_sigmoid_kernel / exp_sigmoid_backward_kernel  elementwise.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "common.h"
#include "launch.h"
#include "profile.h"

namespace ddsp {
namespace fir_grad {

constexpr int kThreads = 256;
constexpr int kTile = 256;              // samples of dL/d audio per block
constexpr int kLdsFloats = 16000;       // 64,000 bytes of static LDS: taps of the tile's frames + the tile of g
constexpr int kChunk = 1024;            // samples of a frame staged at a time by fir_grad_ir_kernel
constexpr int kMaxDesignTaps = 12288;   // grad_ir row of fir_design_backward_kernel in LDS

struct Args {
  int N, F, L, frame_size, start, n_out;
  size_t ir_batch_stride;               // F * L, or 0 when the impulse response is broadcast over the batch
};

__global__ __launch_bounds__(kThreads) void fir_grad_audio_kernel(const float* __restrict__ g, const float* __restrict__ ir,
                                                                  float* __restrict__ grad_audio, Args p) {
  __shared__ float s_mem[kLdsFloats];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int i0 = blockIdx.x * kTile, i1 = min(i0 + kTile, p.N);
  const int f0 = i0 / p.frame_size, f1 = (i1 - 1) / p.frame_size;
  const int n_taps = (f1 - f0 + 1) * p.L;                       // host: n_taps + kTile + L - 1 <= kLdsFloats
  float* s_h = s_mem;
  float* s_g = s_mem + n_taps;
  const float* __restrict__ hb = ir + (size_t)b * p.ir_batch_stride + (size_t)f0 * p.L;
  const float* __restrict__ gb = g + (size_t)b * p.n_out;
  for (int t = tid; t < n_taps; t += kThreads) s_h[t] = hb[t];
  const long j0 = (long)i0 - p.start;                           // g index of (sample i0, tap 0)
  const int n_g = (i1 - i0) + p.L - 1;
  for (int t = tid; t < n_g; t += kThreads) {
    const long j = j0 + t;
    s_g[t] = (j >= 0 && j < (long)p.n_out) ? gb[j] : 0.0f;
  }
  __syncthreads();
  const int i = i0 + tid;
  if (i < i1) {
    const float* __restrict__ h = s_h + (i / p.frame_size - f0) * p.L;
    const float* __restrict__ gw = s_g + tid;
    float acc = 0.0f;
    for (int k = 0; k < p.L; ++k) acc = fmaf(h[k], gw[k], acc);
    grad_audio[(size_t)b * p.N + i] = acc;
  }
}

__global__ __launch_bounds__(kThreads) void fir_grad_audio_any_kernel(const float* __restrict__ g, const float* __restrict__ ir,
                                                                      float* __restrict__ grad_audio, Args p) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.N) return;
  const float* __restrict__ h = ir + (size_t)b * p.ir_batch_stride + (size_t)(i / p.frame_size) * p.L;
  const float* __restrict__ gb = g + (size_t)b * p.n_out;
  const long j0 = (long)i - p.start;
  const long k_lo = max(0L, -j0), k_hi = min((long)p.L, (long)p.n_out - j0);       // 0 <= j0 + k < n_out
  float acc = 0.0f;
  for (long k = k_lo; k < k_hi; ++k) acc = fmaf(h[k], gb[j0 + k], acc);
  grad_audio[(size_t)b * p.N + i] = acc;
}

__global__ __launch_bounds__(kThreads) void fir_grad_ir_kernel(const float* __restrict__ g, const float* __restrict__ audio,
                                                               float* __restrict__ grad_ir, Args p) {
  __shared__ float s_a[kChunk];
  __shared__ float s_g[kChunk + kThreads];
  const int b = blockIdx.z, f = blockIdx.y, tid = threadIdx.x;
  const int k0 = blockIdx.x * kThreads, k = k0 + tid;
  const int ia = f * p.frame_size, ib = min(ia + p.frame_size, p.N);
  const float* __restrict__ ab = audio + (size_t)b * p.N;
  const float* __restrict__ gb = g + (size_t)b * p.n_out;
  float acc = 0.0f;
  for (int c0 = ia; c0 < ib; c0 += kChunk) {
    const int cn = min(kChunk, ib - c0);
    for (int t = tid; t < cn; t += kThreads) s_a[t] = ab[c0 + t];
    const long j0 = (long)c0 + k0 - p.start;                    // g index of (sample c0, tap k0)
    for (int t = tid; t < cn + kThreads - 1; t += kThreads) {
      const long j = j0 + t;
      s_g[t] = (j >= 0 && j < (long)p.n_out) ? gb[j] : 0.0f;
    }
    __syncthreads();
    const float* __restrict__ gw = s_g + tid;
    for (int t = 0; t < cn; ++t) acc = fmaf(s_a[t], gw[t], acc);
    __syncthreads();
  }
  if (k < p.L) grad_ir[((size_t)b * p.F + f) * p.L + k] = acc;
}

// ---- core.sinc_impulse_response ------------------------------------------------------------------------------------------
struct SincArgs { int L, half, high_pass; float scale; };        // c = cutoff * scale (2 / sample_rate, or 1)

// the sums of a block's per-thread fp64 partials, thread 0 adding them in thread order; every thread gets the totals
template <int Q>
__device__ __forceinline__ void block_sums(double (&v)[Q], double* s_part /*[Q * kThreads]*/) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < Q; ++q) s_part[q * kThreads + tid] = v[q];
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      double s = 0.0;
      for (int t = 0; t < kThreads; ++t) s += s_part[q * kThreads + t];
      s_part[q * kThreads] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = s_part[q * kThreads];
}

// x_j = c (j - half) in fp32 as the reference forms it, |x| < 1e-20 replaced by 1e-20; replaced: no gradient reaches c
__device__ __forceinline__ float sinc_arg(float c, int j, int half, bool* replaced) {
  const float x = rn_mul(c, (float)(j - half));
  *replaced = fabsf(x) < 1e-20f;
  return *replaced ? 1e-20f : x;
}
// tf.signal.hamming_window(L): L = 2 half + 1 is odd, and TensorFlow's raised-cosine windows of odd length divide by L - 1
// whatever `periodic` says (window_ops.py, _raised_cosine_window; noise_ir_geom.h has the Hann case); one sample: [1.0]
__device__ __forceinline__ float hamming(int j, int L) {
  return L == 1 ? 1.0f : 0.54f - 0.46f * cospif(2.0f * (float)j / (float)(L - 1));
}
// w_j sin(pi x) / (pi x)
__device__ __forceinline__ float sinc_tap(float c, int j, int half, int L) {
  bool replaced;
  const float x = sinc_arg(c, j, half, &replaced);
  return hamming(j, L) * (sinpif(x) / (3.14159265358979323846f * x));
}

// core.sinc on its own, elementwise
__global__ __launch_bounds__(kThreads) void sinc_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n, float threshold) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
    float x = in[i];
    if (fabsf(x) < threshold) x = threshold;
    out[i] = sinpif(x) / (3.14159265358979323846f * x);
  }
}

__global__ __launch_bounds__(kThreads) void sinc_ir_kernel(const float* __restrict__ cutoff, float* __restrict__ ir, SincArgs p) {
  __shared__ double s_part[kThreads];
  const size_t row = blockIdx.x;
  const float c = rn_mul(cutoff[row], p.scale);
  double v[1] = {0.0};
  for (int j = threadIdx.x; j < p.L; j += kThreads) v[0] += (double)sinc_tap(c, j, p.half, p.L);
  block_sums<1>(v, s_part);
  const float inv = (float)(1.0 / fabs(v[0]));
  for (int j = threadIdx.x; j < p.L; j += kThreads) {
    const float h = sinc_tap(c, j, p.half, p.L) * inv;
    ir[row * p.L + j] = p.high_pass ? (j == p.half ? 1.0f : 0.0f) - h : h;
  }
}

// h_j = n_j / |S|, n_j = w_j s(x_j), S = sum n_j:  dL/dc = (sum G dn - (sum G n) sign(S) S' / |S|) / |S|,  dn_j = w_j s'(x_j) (j - half),
// S' = sum dn_j, G = dL/dh (negated for a high-pass), s'(x) = (pi x cos(pi x) - sin(pi x)) / (pi x^2) - evaluated in fp64: the
// numerator cancels to the third order near x = 0.
__global__ __launch_bounds__(kThreads) void sinc_ir_backward_kernel(const float* __restrict__ cutoff, const float* __restrict__ grad_ir,
                                                                    float* __restrict__ grad_cutoff, SincArgs p) {
  __shared__ double s_part[4 * kThreads];
  const size_t row = blockIdx.x;
  const float c = rn_mul(cutoff[row], p.scale);
  const double pi = 3.14159265358979323846;
  double v[4] = {0.0, 0.0, 0.0, 0.0};                            // S, S', sum G n, sum G dn
  for (int j = threadIdx.x; j < p.L; j += kThreads) {
    bool replaced;
    const double x = (double)sinc_arg(c, j, p.half, &replaced);
    const double w = (double)hamming(j, p.L);
    const double px = pi * x, sn = sin(px), cs = cos(px);
    const double n = w * sn / px;
    const double dn = replaced ? 0.0 : w * (px * cs - sn) / (px * x) * (double)(j - p.half);
    const double G = (double)grad_ir[row * p.L + j];
    v[0] += n; v[1] += dn; v[2] += G * n; v[3] += G * dn;
  }
  block_sums<4>(v, s_part);
  if (threadIdx.x == 0) {
    const double S = v[0], aS = fabs(S), sign = S < 0.0 ? -1.0 : 1.0;
    double d = (v[3] - v[2] * sign * v[1] / aS) / aS;
    if (p.high_pass) d = -d;
    grad_cutoff[row] = (float)(d * (double)p.scale);
  }
}

// ---- the adjoint of the (linear) frequency-sampling design -------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fir_design_backward_kernel(const float* __restrict__ grad_ir /*[R,L]*/,
                                                                       const float* __restrict__ design /*[L,M]*/,
                                                                       float* __restrict__ grad_mag /*[R,M]*/, int M, int L) {
  __shared__ float s_g[kMaxDesignTaps];
  const size_t row = blockIdx.x;
  for (int k = threadIdx.x; k < L; k += kThreads) s_g[k] = grad_ir[row * L + k];
  __syncthreads();
  for (int m = threadIdx.x; m < M; m += kThreads) {
    float acc = 0.0f;
    for (int k = 0; k < L; ++k) acc = fmaf(design[(size_t)k * M + m], s_g[k], acc);
    grad_mag[row * M + m] = acc;
  }
}

__global__ __launch_bounds__(256) void exp_sigmoid_kernel(const float* __restrict__ in,
                                                          float* __restrict__ out, size_t n,
                                                          float log_exponent, float max_value,
                                                          float threshold) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    out[i] = exp_sigmoid(in[i], log_exponent, max_value, threshold);
}

// ---- d exp_sigmoid / dx = log(exponent) (y - threshold) (1 - sigmoid(x)),  y - threshold = max_value sigmoid(x)^log(exponent) ----
__global__ __launch_bounds__(kThreads) void exp_sigmoid_backward_kernel(const float* __restrict__ in, const float* __restrict__ grad_out,
                                                                        float* __restrict__ grad_in, size_t n, float log_exponent,
                                                                        float max_value) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
    const float x = in[i];
    const float e = expf(-fabsf(x));
    const float softplus_neg = (x >= 0.0f) ? log1pf(e) : (-x + log1pf(e));      // log(1 + e^-x) = -log sigmoid(x)
    const float one_minus_sigmoid = (x >= 0.0f) ? e / (1.0f + e) : 1.0f / (1.0f + e);
    grad_in[i] = grad_out[i] * (log_exponent * max_value * expf(-log_exponent * softplus_neg) * one_minus_sigmoid);
  }
}

static int make_args(Args* p, int B, int Bir, int F, int L, int N, int n_out, int start) {
  if (B <= 0 || F <= 0 || L <= 0 || N <= 0 || n_out <= 0 || start < 0) return DDSP_ERR_BAD_SHAPE;
  if (Bir != B && Bir != 1) return DDSP_ERR_BAD_SHAPE;
  if (B > 65535) return DDSP_ERR_UNSUPPORTED;                   // rows ride on a grid axis of 16 bits
  p->N = N; p->F = F; p->L = L; p->start = start; p->n_out = n_out;
  p->frame_size = (N + F - 1) / F;                               // core.py:1446
  if ((N + p->frame_size - 1) / p->frame_size != F) return DDSP_ERR_BAD_SHAPE;   // :1451-1457
  p->ir_batch_stride = (Bir == 1) ? 0 : (size_t)F * L;
  return DDSP_OK;
}

}  // namespace fir_grad
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::fir_grad;

extern "C" int ddsp_fft_convolve_grad_audio_f32(const float* grad_out, const float* impulse_response, float* grad_audio, int B, int Bir,
                                                int F, int L, int N, int n_out, int start, void* stream) {
  if (!grad_out || !impulse_response || !grad_audio) return DDSP_ERR_NULL_POINTER;
  Args p;
  const int rc = make_args(&p, B, Bir, F, L, N, n_out, start);
  if (rc != DDSP_OK) return rc;
  // frames a tile of kTile samples can touch, and what they and the tile of g take in LDS
  const long frames = min((long)F, (long)(kTile - 1) / p.frame_size + 2);
  const long lds_floats = frames * L + kTile + L - 1;
  if (lds_floats <= kLdsFloats) {
    hipLaunchKernelGGL(fir_grad_audio_kernel, dim3((unsigned)((N + kTile - 1) / kTile), (unsigned)B), dim3(kThreads), 0,
                       (hipStream_t)stream, grad_out, impulse_response, grad_audio, p);
  } else {
    hipLaunchKernelGGL(fir_grad_audio_any_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0,
                       (hipStream_t)stream, grad_out, impulse_response, grad_audio, p);
  }
  return check_launch();
}

extern "C" int ddsp_fft_convolve_grad_ir_f32(const float* grad_out, const float* audio, float* grad_impulse_response, int B, int F,
                                             int L, int N, int n_out, int start, void* stream) {
  if (!grad_out || !audio || !grad_impulse_response) return DDSP_ERR_NULL_POINTER;
  Args p;
  const int rc = make_args(&p, B, B, F, L, N, n_out, start);
  if (rc != DDSP_OK) return rc;
  if (F > 65535) return DDSP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fir_grad_ir_kernel, dim3((unsigned)((L + kThreads - 1) / kThreads), (unsigned)F, (unsigned)B), dim3(kThreads), 0,
                     (hipStream_t)stream, grad_out, audio, grad_impulse_response, p);
  return check_launch();
}

static int make_sinc_args(SincArgs* p, size_t rows, int window_size, float sample_rate, int high_pass) {
  if (rows == 0 || rows > (size_t)0x7fffffff || window_size < 0 || sample_rate < 0.0f) return DDSP_ERR_BAD_SHAPE;
  p->half = window_size / 2;
  p->L = 2 * p->half + 1;
  p->high_pass = high_pass ? 1 : 0;
  p->scale = sample_rate > 0.0f ? 2.0f / sample_rate : 1.0f;
  return DDSP_OK;
}

extern "C" int ddsp_sinc_f32(const float* in, float* out, size_t n, float threshold, void* stream) {
  if (!in || !out) return DDSP_ERR_NULL_POINTER;
  if (n == 0) return DDSP_OK;
  const size_t blocks = (n + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(sinc_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(kThreads), 0, (hipStream_t)stream, in, out, n,
                     threshold);
  return check_launch();
}

extern "C" int ddsp_sinc_impulse_response_size(int window_size) { return window_size < 0 ? DDSP_ERR_BAD_SHAPE : 2 * (window_size / 2) + 1; }

extern "C" int ddsp_sinc_impulse_response_f32(const float* cutoff_frequency, float* impulse_response, size_t rows, int window_size,
                                              float sample_rate, int high_pass, void* stream) {
  if (!cutoff_frequency || !impulse_response) return DDSP_ERR_NULL_POINTER;
  SincArgs p;
  const int rc = make_sinc_args(&p, rows, window_size, sample_rate, high_pass);
  if (rc != DDSP_OK) return rc;
  hipLaunchKernelGGL(sinc_ir_kernel, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, cutoff_frequency, impulse_response, p);
  return check_launch();
}

extern "C" int ddsp_sinc_impulse_response_backward_f32(const float* cutoff_frequency, const float* grad_impulse_response,
                                                       float* grad_cutoff_frequency, size_t rows, int window_size, float sample_rate,
                                                       int high_pass, void* stream) {
  if (!cutoff_frequency || !grad_impulse_response || !grad_cutoff_frequency) return DDSP_ERR_NULL_POINTER;
  SincArgs p;
  const int rc = make_sinc_args(&p, rows, window_size, sample_rate, high_pass);
  if (rc != DDSP_OK) return rc;
  hipLaunchKernelGGL(sinc_ir_backward_kernel, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, cutoff_frequency,
                     grad_impulse_response, grad_cutoff_frequency, p);
  return check_launch();
}

extern "C" int ddsp_frequency_impulse_response_backward_f32(const float* grad_impulse_response, const float* design,
                                                            float* grad_magnitudes, size_t rows, int M, int L, void* stream) {
  if (!grad_impulse_response || !design || !grad_magnitudes) return DDSP_ERR_NULL_POINTER;
  if (rows == 0 || rows > (size_t)0x7fffffff || M <= 0 || L <= 0) return DDSP_ERR_BAD_SHAPE;
  if (L > kMaxDesignTaps) return DDSP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(fir_design_backward_kernel, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, grad_impulse_response,
                     design, grad_magnitudes, M, L);
  return check_launch();
}

extern "C" int ddsp_exp_sigmoid_f32(const float* in, float* out, size_t n, float exponent,
                                    float max_value, float threshold, void* stream) {
  if (!in || !out) return DDSP_ERR_NULL_POINTER;
  if (n == 0) return DDSP_OK;
  ProfileScope prof(kExpSigmoid, (hipStream_t)stream);
  hipLaunchKernelGGL(exp_sigmoid_kernel, dim3(grid_for(n, 256 * 8)), dim3(256), 0, (hipStream_t)stream, in,
                     out, n, logf(exponent), max_value, threshold);
  return check_launch();
}

extern "C" int ddsp_exp_sigmoid_backward_f32(const float* in, const float* grad_out, float* grad_in, size_t n, float exponent,
                                             float max_value, float threshold, void* stream) {
  (void)threshold;                                               // an additive constant: it has no part in the derivative
  if (!in || !grad_out || !grad_in) return DDSP_ERR_NULL_POINTER;
  if (n == 0) return DDSP_OK;
  const size_t blocks = (n + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(exp_sigmoid_backward_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(kThreads), 0,
                     (hipStream_t)stream, in, grad_out, grad_in, n, logf(exponent), max_value);
  return check_launch();
}
