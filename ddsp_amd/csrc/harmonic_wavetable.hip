// core.harmonic_distribution_to_wavetable (ddsp/core.py:1217-1235), forward and backward, for tables of L = 64 .. 8192
// points, L a power of two.  The reference pads the K harmonics to L / 2 + 1 real "bins" (bin 0 the DC, zero), casts them to
// complex, runs an irfft and scales by n_wavetable / 2: four passes, 262 MB written at the shipped shape before the
// result's own 262 MB.  In closed form
//   out[r, n] = scale * sum_{k = 1 .. K} w_k hd[r, k - 1] cos(2 pi k n / L),     scale = n_wavetable / L,
// with w_k = 1 except w_{L/2} = 1/2 (a harmonic in the Nyquist bin, K == L / 2) - the adjoint of a real FFT applied to
// real cotangents.  That transform is the one stft_tq_cot_bwd_kernel runs (csrc/spectral_loss_blocks.h): the real
// coefficients go into the packed half-length array the way its cotangents do, with c = (w_k hd_k, 0) and every bin above
// K zero, sl_inverse transforms the G = 8192 / L rows of a block in LDS, and the sample pairs (2 Re U[e], 2 Im U[e])
// leave as 8-byte stores.  Nothing between [rows, K] in and [rows, L] out touches memory.
// Backward: the forward transform.  g[r, :] is loaded unwindowed as sample pairs, sl_forward, the E / O split of
// stft_tq_mag_kernel for bins 1 .. K, grad_hd[r, k - 1] = scale * w_k * Re X[k].
// A row is transformed by itself, in an order that only L decides: the same bits for a row alone and in a batch.
// Other lengths (odd n_wavetable gives L = n_wavetable - 1; sizes that are no power of two) answer DDSP_ERR_UNSUPPORTED;
// the host layer has the general path.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "common.h"
#include "launch.h"
#include "spectral_loss_blocks.h"

namespace ddsp {
namespace harmonic_wavetable {

template <int S>
__global__ __launch_bounds__(kSlThreads) void hd_to_wavetable_kernel(const float* __restrict__ hd, float* __restrict__ out, size_t rows,
                                                                     int K, float scale2 /* 2 * scale */) {
  constexpr int H = S / 2, G = kSlPoints / H, LOG2H = __builtin_ctz(H);
  __shared__ __attribute__((aligned(16))) float2 s[kSlStore];
  const int tid = threadIdx.x;
  const size_t r0 = (size_t)blockIdx.x * G;
  for (int e = tid; e < G * (H / 2 + 1); e += kSlThreads) {      // pairs of bins (k, H - k), k = 0 .. H / 2
    const int g = e / (H / 2 + 1), k = e - g * (H / 2 + 1);
    if (r0 + g >= rows) continue;
    const int pa = g * H + sl_pos<H>(k), pb = g * H + sl_pos<H>((H - k) & (H - 1));
    const float rev = (float)k * (1.0f / (float)S);
    const float c = __builtin_amdgcn_cosf(rev), sn = __builtin_amdgcn_sinf(rev);
    const float* __restrict__ row = hd + (r0 + g) * (size_t)K;
    auto coefficient = [&](int bin) {                             // w_bin hd[bin - 1]; bins 0 and above K are zero
      if (bin == 0 || bin > K) return 0.0f;
      return bin == H ? 0.5f * row[bin - 1] : row[bin - 1];
    };
    float c1 = coefficient(k), c2 = coefficient(H - k);
    if (k == 0) {                                                 // bins 0 and L / 2
      s[SP(pa)] = make_float2(0.5f * (c1 + c2), 0.5f * (c1 - c2));
    } else {
      if (2 * k == H) c2 = c1;                                    // the self-paired bin L / 4
      c1 *= 0.5f;
      c2 *= 0.5f;
      const float gx = 0.5f * (c1 + c2), dx = 0.5f * (c1 - c2);
      const float qx = dx * c, qy = dx * sn;                      // D * (c + i sn), D real
      s[SP(pa)] = make_float2(gx - qy, qx);
      if (2 * k != H) s[SP(pb)] = make_float2(gx + qy, qx);
    }
  }
  __syncthreads();
  sl_inverse<H>(s, tid, G, 0);
  __syncthreads();
  const bool vec = (reinterpret_cast<uintptr_t>(out) & 7) == 0;  // (a row starts an even number of floats in)
  for (int it = tid; it < G * H; it += kSlThreads) {
    const int g = it >> LOG2H, e = it & (H - 1);
    if (r0 + g >= rows) continue;
    const float2 u = s[SP(it)];
    float* __restrict__ dst = out + (r0 + g) * (size_t)S + 2 * e;
    if (vec) {
      *reinterpret_cast<float2*>(dst) = make_float2(scale2 * u.x, scale2 * u.y);
    } else {
      dst[0] = scale2 * u.x;
      dst[1] = scale2 * u.y;
    }
  }
}

template <int S>
__global__ __launch_bounds__(kSlThreads) void hd_to_wavetable_bwd_kernel(const float* __restrict__ grad_out, float* __restrict__ grad_hd,
                                                                         size_t rows, int K, FastDiv div_k, float scale) {
  constexpr int H = S / 2, G = kSlPoints / H, LOG2H = __builtin_ctz(H);
  __shared__ __attribute__((aligned(16))) float2 s[kSlStore];
  const int tid = threadIdx.x;
  const size_t r0 = (size_t)blockIdx.x * G;
  const bool vec = (reinterpret_cast<uintptr_t>(grad_out) & 7) == 0;
  for (int it = tid; it < G * H; it += kSlThreads) {
    const int g = it >> LOG2H, e = it & (H - 1);
    float2 v = make_float2(0.0f, 0.0f);
    if (r0 + g < rows) {
      const float* __restrict__ src = grad_out + (r0 + g) * (size_t)S + 2 * e;
      if (vec) v = *reinterpret_cast<const float2*>(src);
      else v = make_float2(src[0], src[1]);
    }
    s[SP(it)] = v;
  }
  __syncthreads();
  sl_forward<H>(s, tid, G, 0);
  __syncthreads();
  for (int e = tid; e < G * K; e += kSlThreads) {                // bins 1 .. K of every row
    uint32_t kk;
    const int g = (int)fastdiv((uint32_t)e, div_k, kk);
    if (r0 + g >= rows) continue;
    const int k = (int)kk + 1;
    const int ia = sl_pos<H>(k & (H - 1)), ib = sl_pos<H>((H - k) & (H - 1));
    const float rev = (float)k * (1.0f / (float)S);
    const float c = __builtin_amdgcn_cosf(rev), sn = __builtin_amdgcn_sinf(rev);
    const float2 za = s[SP(g * H + ia)], zb = s[SP(g * H + ib)];
    const float ex = 0.5f * (za.x + zb.x);                                  // E = (Za + conj Zb) / 2
    const float ox = 0.5f * (za.y + zb.y), oy = -0.5f * (za.x - zb.x);      // O = (Za - conj Zb) / 2i
    const float xr = ex + fmaf(ox, c, oy * sn);                             // Re (E + (c - i sn) O)
    grad_hd[(r0 + g) * (size_t)K + kk] = (k == H ? 0.5f * scale : scale) * xr;
  }
}

static bool supported(int L) { return L >= 64 && L <= 2 * kSlPoints && (L & (L - 1)) == 0; }

}  // namespace harmonic_wavetable
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::harmonic_wavetable;

#define DDSP_HW_SIZES(X) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096) X(8192)

extern "C" int ddsp_harmonic_wavetable_f32(const float* hd, float* out, size_t rows, int K, int L, float scale, void* stream) {
  if (!hd || !out) return DDSP_ERR_NULL_POINTER;
  if (K < 1 || L < 2 || (L & 1) || K > L / 2) return DDSP_ERR_BAD_SHAPE;
  if (!supported(L)) return DDSP_ERR_UNSUPPORTED;
  const size_t per_block = (size_t)(2 * kSlPoints / L), blocks = (rows + per_block - 1) / per_block;
  if (blocks > (size_t)0x7FFFFFFF) return DDSP_ERR_UNSUPPORTED;
  if (rows == 0) return DDSP_OK;
  hipStream_t st = (hipStream_t)stream;
  switch (L) {
#define DDSP_HW_CASE(SZ) case SZ: hipLaunchKernelGGL((hd_to_wavetable_kernel<SZ>), dim3((unsigned)blocks), dim3(kSlThreads), 0, st, hd, out, \
                                                      rows, K, 2.0f * scale); break;
    DDSP_HW_SIZES(DDSP_HW_CASE)
#undef DDSP_HW_CASE
    default: return DDSP_ERR_UNSUPPORTED;
  }
  return check_launch();
}

extern "C" int ddsp_harmonic_wavetable_backward_f32(const float* grad_out, float* grad_hd, size_t rows, int K, int L, float scale,
                                                    void* stream) {
  if (!grad_out || !grad_hd) return DDSP_ERR_NULL_POINTER;
  if (K < 1 || L < 2 || (L & 1) || K > L / 2) return DDSP_ERR_BAD_SHAPE;
  if (!supported(L)) return DDSP_ERR_UNSUPPORTED;
  const size_t per_block = (size_t)(2 * kSlPoints / L), blocks = (rows + per_block - 1) / per_block;
  if (blocks > (size_t)0x7FFFFFFF) return DDSP_ERR_UNSUPPORTED;
  if (rows == 0) return DDSP_OK;
  hipStream_t st = (hipStream_t)stream;
  const FastDiv div_k = make_fastdiv((uint32_t)K);
  switch (L) {
#define DDSP_HW_CASE(SZ) case SZ: hipLaunchKernelGGL((hd_to_wavetable_bwd_kernel<SZ>), dim3((unsigned)blocks), dim3(kSlThreads), 0, st, \
                                                      grad_out, grad_hd, rows, K, div_k, scale); break;
    DDSP_HW_SIZES(DDSP_HW_CASE)
#undef DDSP_HW_CASE
    default: return DDSP_ERR_UNSUPPORTED;
  }
  return check_launch();
}
