// The hand-written part of ddsp/training/decoders.py RnnFcDecoder for gfx950 (C ABI: decoder_abi.h).  The matrix products
// whose M is batch * time (Dense layers, the GRU's input projection, the weight gradients) are the framework's; here is what
// it does badly:
//
//   1. norm_fwd_kernel / norm_bwd_kernel   bias + Keras LayerNormalization (eps inside the root, biased two-pass variance)
//                            + activation.  A wavefront per row, lanes over channels; rows of up to 512 channels stay in
//                            registers between the passes, wider ones are re-read.  A row of equal values has mean = that value
//                            exactly, so xhat = 0.  The backward gives dx in one visit of the row; dgamma, dbeta and dbias are
//                            partial rows per WAVEFRONT (registers, or its own slab row for wide layers), summed in ascending
//                            order by norm_reduce_kernel.
//   2. gru_fwd_*_kernel      ONE launch per time step - the step boundary is the kernel boundary; there is no grid barrier and
//                            nothing polls memory.  A block owns 16 hidden units for the three gates and all batch rows; its four
//                            wavefronts take 16-row tiles in turn.  h_{t-1} comes straight from y[:, t - 1] (h0 at t = 0), is
//                            split into fp16 hi / lo on the fly and multiplied by the block's columns of the recurrent matrix,
//                            which gru_pack_kernel split ONCE per call into MFMA fragments (power-of-two normalised by the
//                            matrix's largest magnitude; K tails zero).  hi hi + hi lo + lo hi as in split_f16.h.  The epilogue
//                            does the gate arithmetic and writes y[:, t] and, when asked, z, r, hh and mh_h.
//   3. gru_bwd_*_kernel      t = T-1 .. 0.  dh_t is complete in one of two [batch, hidden] buffers.  Every block forms the
//                            recurrent-side gate gradients d_rec = (da_z, da_r, da_h r) of ALL 3 H columns as MFMA A fragments
//                            (elementwise, cheap; normalised per batch row by their largest magnitude, found in a first visit),
//                            multiplies by its 16 rows of the recurrent matrix (transposed fragments) and writes its slice of
//                            dh_{t-1} = dh_t z + d_rec R^T + dy_{t-1} into the other buffer, and its slice of d_in / d_rec.
//   The *_plain_kernel pair is the vector-ALU form of last resort for hidden sizes that are no multiple of 16.
//
// No atomics; every sum has a fixed order; a batch row's values depend on that row alone: the same bits on every run and for
// any subset of rows (the parameter-gradient partials of the norm depend on the row COUNT, as any batch sum does).
// Limits (DDSP_ERR_UNSUPPORTED beyond): hidden <= 2048, batch * hidden < 2^31, channels < 2^24.  The initial state must lie
// inside fp16's range (|h0| < 65504) on the MFMA path: every later state is a convex mix of it and a tanh.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "decoder_abi.h"
#include "common.h"
#include "launch.h"
#include "split_f16.h"

namespace ddsp {
namespace decoder {

constexpr int kSmallCh = 512;              // channels a wavefront keeps in registers: 8 per lane
constexpr int kPerLane = kSmallCh / 64;
constexpr unsigned kNormBwdBlocks = 256;   // at most this many blocks (x 4 wavefronts) of partial rows
constexpr int kMaxPartials = 64;           // blocks of gru_max_kernel
constexpr size_t kHeaderBytes = 512;       // workspace: int exponent at 0, kMaxPartials floats at 256

// ---- activations ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float a) { return 1.0f / (1.0f + expf(-a)); }

__device__ __forceinline__ float act_fwd(float u, int act) {
  switch (act) {
    case DDSP_ACT_LEAKY_RELU: return u > 0.0f ? u : 0.2f * u;
    case DDSP_ACT_RELU: return relu_keep_nan(u);
    case DDSP_ACT_SIGMOID: return sigmoidf_(u);
    case DDSP_ACT_TANH: return tanhf(u);
    default: return u;
  }
}
__device__ __forceinline__ float act_grad(float u, int act) {
  switch (act) {
    case DDSP_ACT_LEAKY_RELU: return u > 0.0f ? 1.0f : 0.2f;
    case DDSP_ACT_RELU: return u > 0.0f ? 1.0f : 0.0f;
    case DDSP_ACT_SIGMOID: { const float s = sigmoidf_(u); return s * (1.0f - s); }
    case DDSP_ACT_TANH: { const float t = tanhf(u); return 1.0f - t * t; }
    default: return 1.0f;
  }
}

// ---- 1. bias + LayerNorm + activation -------------------------------------------------------------------------------
template <bool SMALL>
__global__ __launch_bounds__(256) void norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ y, float* __restrict__ xhat, float* __restrict__ rstd_out,
                                                       size_t rows, int ch, int act, float eps) {
  const int lane = threadIdx.x & 63;
  const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (size_t)gridDim.x * 4;
  const float inv_ch = 1.0f / (float)ch;
  for (size_t row = wave; row < rows; row += n_waves) {
    const float* xr = x + row * (size_t)ch;
    float v[kPerLane];
    float s = 0.0f, lo = INFINITY, hi = -INFINITY;
    if (SMALL) {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        const int c = lane + 64 * k;
        v[k] = c < ch ? xr[c] + bias[c] : 0.0f;
        if (c < ch) { s += v[k]; lo = fminf(lo, v[k]); hi = fmaxf(hi, v[k]); }
      }
    } else {
      for (int c = lane; c < ch; c += 64) {
        const float a = xr[c] + bias[c];
        s += a; lo = fminf(lo, a); hi = fmaxf(hi, a);
      }
    }
    s = wave_sum(s); lo = wave_min(lo); hi = wave_max(hi);
    const float mean = lo == hi ? lo : s * inv_ch;
    float q = 0.0f;
    if (SMALL) {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        const float d = v[k] - mean;
        if (lane + 64 * k < ch) q = fmaf(d, d, q);
      }
    } else {
      for (int c = lane; c < ch; c += 64) {
        const float d = (xr[c] + bias[c]) - mean;
        q = fmaf(d, d, q);
      }
    }
    q = wave_sum(q);
    const float rstd = 1.0f / sqrtf(q * inv_ch + eps);
    float* yr = y + row * (size_t)ch;
    float* hr = xhat ? xhat + row * (size_t)ch : nullptr;
    if (SMALL) {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        const int c = lane + 64 * k;
        if (c < ch) {
          const float h = (v[k] - mean) * rstd;
          yr[c] = act_fwd(fmaf(gamma[c], h, beta[c]), act);
          if (hr) hr[c] = h;
        }
      }
    } else {
      for (int c = lane; c < ch; c += 64) {
        const float h = ((xr[c] + bias[c]) - mean) * rstd;
        yr[c] = act_fwd(fmaf(gamma[c], h, beta[c]), act);
        if (hr) hr[c] = h;
      }
    }
    if (rstd_out && lane == 0) rstd_out[row] = rstd;
  }
}

// slab: [n_waves][3][ch] = this wavefront's sums of (du xhat, du, dx) over its rows
template <bool SMALL>
__global__ __launch_bounds__(256) void norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ xhat,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ dx, float* __restrict__ slab,
                                                       size_t rows, int ch, int act) {
  const int lane = threadIdx.x & 63;
  const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (size_t)gridDim.x * 4;
  const float inv_ch = 1.0f / (float)ch;
  float* mine = slab + wave * 3 * (size_t)ch;      // a lane touches its own columns only
  float ag[kPerLane], ab[kPerLane], ax[kPerLane];
  if (SMALL) {
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) ag[k] = ab[k] = ax[k] = 0.0f;
  } else {
    for (int c = lane; c < ch; c += 64) mine[c] = mine[ch + c] = mine[2 * (size_t)ch + c] = 0.0f;
  }
  for (size_t row = wave; row < rows; row += n_waves) {
    const float* dyr = dy + row * (size_t)ch;
    const float* hr = xhat + row * (size_t)ch;
    float* dxr = dx + row * (size_t)ch;
    const float rs = rstd[row];
    float g[kPerLane], h[kPerLane];
    float s1 = 0.0f, s2 = 0.0f;
    if (SMALL) {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        const int c = lane + 64 * k;
        g[k] = h[k] = 0.0f;
        if (c < ch) {
          h[k] = hr[c];
          const float du = dyr[c] * act_grad(fmaf(gamma[c], h[k], beta[c]), act);
          ag[k] = fmaf(du, h[k], ag[k]);
          ab[k] += du;
          g[k] = du * gamma[c];
          s1 += g[k];
          s2 = fmaf(g[k], h[k], s2);
        }
      }
    } else {
      for (int c = lane; c < ch; c += 64) {
        const float hv = hr[c];
        const float du = dyr[c] * act_grad(fmaf(gamma[c], hv, beta[c]), act);
        mine[c] = fmaf(du, hv, mine[c]);
        mine[ch + c] += du;
        const float gv = du * gamma[c];
        s1 += gv;
        s2 = fmaf(gv, hv, s2);
      }
    }
    s1 = wave_sum(s1) * inv_ch;
    s2 = wave_sum(s2) * inv_ch;
    if (SMALL) {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        const int c = lane + 64 * k;
        if (c < ch) {
          const float d = rs * ((g[k] - s1) - h[k] * s2);
          dxr[c] = d;
          ax[k] += d;
        }
      }
    } else {
      for (int c = lane; c < ch; c += 64) {
        const float hv = hr[c];
        const float gv = dyr[c] * act_grad(fmaf(gamma[c], hv, beta[c]), act) * gamma[c];
        const float d = rs * ((gv - s1) - hv * s2);
        dxr[c] = d;
        mine[2 * (size_t)ch + c] += d;
      }
    }
  }
  if (SMALL) {
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const int c = lane + 64 * k;
      if (c < ch) { mine[c] = ag[k]; mine[ch + c] = ab[k]; mine[2 * (size_t)ch + c] = ax[k]; }
    }
  }
}

// dparams[i] = sum over the wavefronts' partial rows, ascending; i over 3 ch
__global__ __launch_bounds__(256) void norm_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dparams, size_t n_waves,
                                                          int ch3) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= ch3) return;
  float s = 0.0f;
  for (size_t w = 0; w < n_waves; ++w) s += slab[w * (size_t)ch3 + i];
  dparams[i] = s;
}

static inline unsigned norm_bwd_blocks(size_t rows) {
  const size_t b = (rows + 3) / 4;
  return (unsigned)(b < 1 ? 1 : (b > kNormBwdBlocks ? kNormBwdBlocks : b));
}

// ---- 2. / 3. the GRU -------------------------------------------------------------------------------------------------
// largest magnitude of the recurrent matrix: a partial per block, in a fixed slot (max is order independent anyway)
__global__ __launch_bounds__(256) void gru_max_kernel(const float* __restrict__ r, size_t n, float* __restrict__ partials) {
  __shared__ float lds[4];
  float m = 0.0f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(r[i]));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
}

// MFMA B fragments of the recurrent matrix R [H, 3 H], scaled by 2^-e, as fp16 hi / lo:
//   fragment (g, jt, ks), part p at u32x4 index ((((g JT + jt) KS + ks) 2 + p) 64 + lane; lane l, element q holds
//   forward     B[k][j] = R[ks 32 + k][g H + jt 16 + j]      (mh = h R: K runs over the rows of R)
//   transposed  B[k][j] = R[jt 16 + j][g H + ks 32 + k]      (dh = d_rec R^T: K runs over the columns of gate g)
//   with k = 8 (l / 16) + q, j = l % 16, and 0 where ks 32 + k >= H.
__global__ __launch_bounds__(256) void gru_pack_kernel(const float* __restrict__ r, const float* __restrict__ partials, int* __restrict__ exponent,
                                                       u32x4* __restrict__ packed, int H, int transposed) {
  const int JT = H / 16, KS = (H + 31) / 32;
  float m = 0.0f;
  for (int i = 0; i < kMaxPartials; ++i) m = fmaxf(m, partials[i]);
  const int e = pow2_exponent(m);
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id == 0) *exponent = e;
  const size_t frag_id = id >> 6;
  if (frag_id >= (size_t)3 * JT * KS) return;
  const int lane = (int)(id & 63);
  const int ks = (int)(frag_id % KS), jt = (int)((frag_id / KS) % JT), g = (int)(frag_id / ((size_t)KS * JT));
  const int j = lane & 15, k0 = ks * 32 + 8 * (lane >> 4);
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int k = k0 + q;
    float a = 0.0f;
    if (k < H) a = transposed ? r[(size_t)(jt * 16 + j) * 3 * H + (size_t)g * H + k] : r[(size_t)k * 3 * H + (size_t)g * H + jt * 16 + j];
    v[q] = ldexpf(a, -e);
  }
  store_fragment(packed, frag_id, lane, v);
}

// the gate arithmetic of one (row, unit) at step t, and everything that is written for it
__device__ __forceinline__ void gate_forward(float mh_z, float mh_r, float mh_h, const float* __restrict__ mx, float h_prev,
                                             float* __restrict__ y, float* __restrict__ saved, size_t plane, size_t row_t, int H, int u) {
  const float* m = mx + row_t * 3 * (size_t)H;
  const float z = sigmoidf_(m[u] + mh_z);
  const float r = sigmoidf_(m[H + u] + mh_r);
  const float hh = tanhf(fmaf(r, mh_h, m[2 * H + u]));
  const size_t at = row_t * (size_t)H + u;
  y[at] = fmaf(z, h_prev - hh, hh);                // z h + (1 - z) hh
  if (saved) {
    saved[at] = z;
    saved[plane + at] = r;
    saved[2 * plane + at] = hh;
    saved[3 * plane + at] = mh_h;
  }
}

__global__ __launch_bounds__(256) void gru_fwd_mfma_kernel(const float* __restrict__ mx, const u32x4* __restrict__ packed,
                                                           const int* __restrict__ exponent, const float* __restrict__ bias,
                                                           const float* __restrict__ h_prev, size_t h_stride, float* __restrict__ y,
                                                           float* __restrict__ saved, int B, int T, int H, int t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jt = blockIdx.x, JT = H / 16, KS = (H + 31) / 32;
  const float scale = ldexpf(1.0f, *exponent);
  const size_t plane = (size_t)B * T * H;
  const int tiles = (B + 15) / 16;
  for (int tile = wave; tile < tiles; tile += 4) {                  // wave-uniform: an MFMA needs all 64 lanes
    const int a_row = tile * 16 + (lane & 15), kq = 8 * (lane >> 4);
    const float* hp = h_prev + (size_t)(a_row < B ? a_row : 0) * h_stride;
    f32x4 acc[3], cross[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = cross[g] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (int ks = 0; ks < KS; ++ks) {
      const int k = ks * 32 + kq;
      float hv[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (a_row < B && k < H) {                                     // H % 8 == 0: k < H means k + 7 < H
        const PackedF4 p0 = *reinterpret_cast<const PackedF4*>(hp + k), p1 = *reinterpret_cast<const PackedF4*>(hp + k + 4);
        hv[0] = p0.x; hv[1] = p0.y; hv[2] = p0.z; hv[3] = p0.w; hv[4] = p1.x; hv[5] = p1.y; hv[6] = p1.z; hv[7] = p1.w;
      }
      f16x8 a_hi, a_lo;
      split8(hv, a_hi, a_lo);
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const size_t at = (((size_t)g * JT + jt) * KS + ks) * 128 + lane;
        const f16x8 b_hi = __builtin_bit_cast(f16x8, packed[at]), b_lo = __builtin_bit_cast(f16x8, packed[at + 64]);
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_hi, acc[g], 0, 0, 0);
        cross[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_lo, cross[g], 0, 0, 0);
        cross[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, b_hi, cross[g], 0, 0, 0);
      }
    }
    const int u = jt * 16 + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = tile * 16 + 4 * (lane >> 4) + q;
      if (row < B) {
        const float mh_z = fmaf(combine(acc[0][q], cross[0][q]), scale, bias[u]);
        const float mh_r = fmaf(combine(acc[1][q], cross[1][q]), scale, bias[H + u]);
        const float mh_h = fmaf(combine(acc[2][q], cross[2][q]), scale, bias[2 * H + u]);
        gate_forward(mh_z, mh_r, mh_h, mx, h_prev[(size_t)row * h_stride + u], y, saved, plane, (size_t)row * T + t, H, u);
      }
    }
  }
}

__global__ __launch_bounds__(256) void gru_fwd_plain_kernel(const float* __restrict__ mx, const float* __restrict__ rk,
                                                            const float* __restrict__ bias, const float* __restrict__ h_prev,
                                                            size_t h_stride, float* __restrict__ y, float* __restrict__ saved, int B, int T,
                                                            int H, int t) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (size_t)B * H) return;
  const int row = (int)(id / H), u = (int)(id % H);
  const float* hp = h_prev + (size_t)row * h_stride;
  float az = 0.0f, ar = 0.0f, ah = 0.0f;
  for (int k = 0; k < H; ++k) {
    const float hv = hp[k];
    const float* rr = rk + (size_t)k * 3 * H;
    az = fmaf(hv, rr[u], az);
    ar = fmaf(hv, rr[H + u], ar);
    ah = fmaf(hv, rr[2 * H + u], ah);
  }
  gate_forward(az + bias[u], ar + bias[H + u], ah + bias[2 * H + u], mx, hp[u], y, saved, (size_t)B * T * H, (size_t)row * T + t, H, u);
}

// the pre-activation gradients of one (row, unit) from the complete dh_t
struct GateGrad { float z, r, h, rec_h; };      // da_z, da_r, da_h, da_h r
__device__ __forceinline__ GateGrad gate_grad(float dh, float z, float r, float hh, float mh_h, float h_prev) {
  GateGrad d;
  d.h = dh * (1.0f - z) * (1.0f - hh * hh);
  d.z = dh * (h_prev - hh) * z * (1.0f - z);
  d.r = d.h * mh_h * r * (1.0f - r);
  d.rec_h = d.h * r;
  return d;
}
__device__ __forceinline__ GateGrad gate_grad_at(const float* __restrict__ dh, const float* __restrict__ saved, size_t plane,
                                                 const float* __restrict__ h_prev, size_t h_stride, size_t row, size_t row_t, int H, int u) {
  const size_t at = row_t * (size_t)H + u;
  return gate_grad(dh[row * (size_t)H + u], saved[at], saved[plane + at], saved[2 * plane + at], saved[3 * plane + at],
                   h_prev[row * h_stride + u]);
}
// what a (row, unit) writes at step t: its entries of d_in and d_rec, and dh_{t-1}
__device__ __forceinline__ void gate_backward_store(const GateGrad& d, float carried, const float* __restrict__ dh, const float* __restrict__ saved,
                                                    const float* __restrict__ dy_prev, size_t dy_stride, float* __restrict__ d_in,
                                                    float* __restrict__ d_rec, float* __restrict__ dh_out, size_t row, size_t row_t, int H, int u) {
  const size_t at3 = row_t * 3 * (size_t)H + u;
  d_in[at3] = d.z; d_in[at3 + H] = d.r; d_in[at3 + 2 * (size_t)H] = d.h;
  d_rec[at3] = d.z; d_rec[at3 + H] = d.r; d_rec[at3 + 2 * (size_t)H] = d.rec_h;
  float out = fmaf(dh[row * (size_t)H + u], saved[row_t * (size_t)H + u], carried);
  if (dy_prev) out += dy_prev[row * dy_stride + u];
  dh_out[row * (size_t)H + u] = out;
}

__global__ __launch_bounds__(256) void gru_bwd_mfma_kernel(const float* __restrict__ dh, const float* __restrict__ saved,
                                                           const u32x4* __restrict__ packed, const int* __restrict__ exponent,
                                                           const float* __restrict__ h_prev, size_t h_stride, const float* __restrict__ dy_prev,
                                                           size_t dy_stride, float* __restrict__ d_in, float* __restrict__ d_rec,
                                                           float* __restrict__ dh_out, int B, int T, int H, int t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jt = blockIdx.x, JT = H / 16, KS = (H + 31) / 32;
  const int e_r = *exponent;
  const size_t plane = (size_t)B * T * H;
  const int tiles = (B + 15) / 16;
  for (int tile = wave; tile < tiles; tile += 4) {
    const int a_row = tile * 16 + (lane & 15), kq = 8 * (lane >> 4);
    const bool live = a_row < B;
    const size_t row_t = (size_t)(live ? a_row : 0) * T + t;
    // first visit: the largest magnitude of each row's d_rec, for the power-of-two normalisation ahead of the fp16 split
    float m = 0.0f;
    for (int ks = 0; ks < KS; ++ks) {
      const int k = ks * 32 + kq;
      if (live && k < H) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const GateGrad d = gate_grad_at(dh, saved, plane, h_prev, h_stride, (size_t)a_row, row_t, H, k + q);
          m = fmaxf(m, fmaxf(fabsf(d.z), fmaxf(fabsf(d.r), fabsf(d.rec_h))));
        }
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16));                                  // the four lanes that hold row lane % 16
    m = fmaxf(m, __shfl_xor(m, 32));
    const int e_d = pow2_exponent(m);                                 // per ROW: a row's bits do not depend on its neighbours
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f}, cross = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ks = 0; ks < KS; ++ks) {
      const int k = ks * 32 + kq;
      float vz[8], vr[8], vh[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) vz[q] = vr[q] = vh[q] = 0.0f;
      if (live && k < H) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const GateGrad d = gate_grad_at(dh, saved, plane, h_prev, h_stride, (size_t)a_row, row_t, H, k + q);
          vz[q] = ldexpf(d.z, -e_d); vr[q] = ldexpf(d.r, -e_d); vh[q] = ldexpf(d.rec_h, -e_d);
        }
      }
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        f16x8 a_hi, a_lo;
        split8(g == 0 ? vz : (g == 1 ? vr : vh), a_hi, a_lo);
        const size_t at = (((size_t)g * JT + jt) * KS + ks) * 128 + lane;
        const f16x8 b_hi = __builtin_bit_cast(f16x8, packed[at]), b_lo = __builtin_bit_cast(f16x8, packed[at + 64]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_hi, acc, 0, 0, 0);
        cross = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_lo, cross, 0, 0, 0);
        cross = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, b_hi, cross, 0, 0, 0);
      }
    }
    const int u = jt * 16 + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = tile * 16 + 4 * (lane >> 4) + q;
      const int e_row = __shfl(e_d, 4 * (lane >> 4) + q);
      if (row < B) {
        const size_t rt = (size_t)row * T + t;
        const GateGrad d = gate_grad_at(dh, saved, plane, h_prev, h_stride, (size_t)row, rt, H, u);
        gate_backward_store(d, ldexpf(combine(acc[q], cross[q]), e_row + e_r), dh, saved, dy_prev, dy_stride, d_in, d_rec, dh_out,
                            (size_t)row, rt, H, u);
      }
    }
  }
}

__global__ __launch_bounds__(256) void gru_bwd_plain_kernel(const float* __restrict__ dh, const float* __restrict__ saved,
                                                            const float* __restrict__ rk, const float* __restrict__ h_prev, size_t h_stride,
                                                            const float* __restrict__ dy_prev, size_t dy_stride, float* __restrict__ d_in,
                                                            float* __restrict__ d_rec, float* __restrict__ dh_out, int B, int T, int H, int t) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (size_t)B * H) return;
  const size_t row = id / H;
  const int k = (int)(id % H);
  const size_t plane = (size_t)B * T * H, row_t = row * T + t;
  const float* rr = rk + (size_t)k * 3 * H;
  float acc = 0.0f;
  for (int u = 0; u < H; ++u) {
    const GateGrad d = gate_grad_at(dh, saved, plane, h_prev, h_stride, row, row_t, H, u);
    acc = fmaf(d.z, rr[u], acc);
    acc = fmaf(d.r, rr[H + u], acc);
    acc = fmaf(d.rec_h, rr[2 * H + u], acc);
  }
  const GateGrad d = gate_grad_at(dh, saved, plane, h_prev, h_stride, row, row_t, H, k);
  gate_backward_store(d, acc, dh, saved, dy_prev, dy_stride, d_in, d_rec, dh_out, row, row_t, H, k);
}

// dh_{T-1} = dy[:, T - 1]
__global__ __launch_bounds__(256) void gru_bwd_init_kernel(const float* __restrict__ dy, float* __restrict__ dh, int B, int T, int H) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (size_t)B * H) return;
  const size_t row = id / H, u = id % H;
  dh[id] = dy[(row * T + (T - 1)) * (size_t)H + u];
}

static inline size_t packed_bytes(int H) {
  if (H % 16 != 0) return 0;
  return (size_t)3 * (H / 16) * ((H + 31) / 32) * 128 * sizeof(u32x4);
}
static inline bool gru_supported(int B, int H) {
  return H <= DDSP_GRU_MAX_HIDDEN && (size_t)B * (size_t)H < ((size_t)1 << 31);
}
// the prep of one call: the matrix's exponent and its fragments
static inline void gru_prepare(const float* rk, char* ws, int H, int transposed, hipStream_t stream) {
  float* partials = reinterpret_cast<float*>(ws + 256);
  int* exponent = reinterpret_cast<int*>(ws);
  hipLaunchKernelGGL(gru_max_kernel, dim3(kMaxPartials), dim3(256), 0, stream, rk, (size_t)3 * H * H, partials);
  const size_t threads = (size_t)3 * (H / 16) * ((H + 31) / 32) * 64;
  hipLaunchKernelGGL(gru_pack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, rk, partials, exponent,
                     reinterpret_cast<u32x4*>(ws + kHeaderBytes), H, transposed);
}

}  // namespace decoder
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::decoder;

extern "C" int ddsp_bias_norm_act_f32(const float* x, const float* bias, const float* gamma, const float* beta, float* y, float* xhat,
                                      float* rstd, size_t rows, int ch, int act, float eps, void* stream) {
  if (!x || !bias || !gamma || !beta || !y || (xhat == nullptr) != (rstd == nullptr)) return DDSP_ERR_NULL_POINTER;
  if (ch < 1 || act < DDSP_ACT_LINEAR || act > DDSP_ACT_TANH || !(eps >= 0.0f)) return DDSP_ERR_BAD_SHAPE;
  if (ch >= (1 << 24)) return DDSP_ERR_UNSUPPORTED;
  if (rows == 0) return DDSP_OK;
  const size_t blocks = (rows + 3) / 4;
  const dim3 grid((unsigned)(blocks > 65536 ? 65536 : blocks));
  if (ch <= kSmallCh)
    hipLaunchKernelGGL(norm_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, bias, gamma, beta, y, xhat, rstd, rows, ch, act, eps);
  else
    hipLaunchKernelGGL(norm_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, bias, gamma, beta, y, xhat, rstd, rows, ch, act, eps);
  return check_launch();
}

extern "C" size_t ddsp_bias_norm_act_backward_workspace_bytes(size_t rows, int ch) {
  if (ch < 1 || rows == 0) return 0;
  return (size_t)norm_bwd_blocks(rows) * 4 * 3 * (size_t)ch * sizeof(float);
}

extern "C" int ddsp_bias_norm_act_backward_f32(const float* dy, const float* xhat, const float* rstd, const float* gamma,
                                               const float* beta, float* dx, float* dparams, void* workspace, size_t workspace_bytes,
                                               size_t rows, int ch, int act, void* stream) {
  if (!dy || !xhat || !rstd || !gamma || !beta || !dx || !dparams) return DDSP_ERR_NULL_POINTER;
  if (ch < 1 || act < DDSP_ACT_LINEAR || act > DDSP_ACT_TANH) return DDSP_ERR_BAD_SHAPE;
  if (ch >= (1 << 24)) return DDSP_ERR_UNSUPPORTED;
  if (rows == 0) return hipMemsetAsync(dparams, 0, 3 * (size_t)ch * sizeof(float), (hipStream_t)stream) == hipSuccess ? DDSP_OK : DDSP_ERR_LAUNCH;
  if (!workspace) return DDSP_ERR_NULL_POINTER;
  if (workspace_bytes < ddsp_bias_norm_act_backward_workspace_bytes(rows, ch)) return DDSP_ERR_WORKSPACE;
  const unsigned blocks = norm_bwd_blocks(rows);
  float* slab = static_cast<float*>(workspace);
  if (ch <= kSmallCh)
    hipLaunchKernelGGL(norm_bwd_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, xhat, rstd, gamma, beta, dx, slab, rows, ch, act);
  else
    hipLaunchKernelGGL(norm_bwd_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, xhat, rstd, gamma, beta, dx, slab, rows, ch, act);
  hipLaunchKernelGGL(norm_reduce_kernel, dim3((unsigned)((3 * ch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, slab, dparams,
                     (size_t)blocks * 4, 3 * ch);
  return check_launch();
}

extern "C" size_t ddsp_gru_forward_workspace_bytes(int batch, int hidden) {
  if (batch < 1 || hidden < 1 || !gru_supported(batch, hidden)) return 0;
  return kHeaderBytes + packed_bytes(hidden);
}

extern "C" int ddsp_gru_forward_f32(const float* mx, const float* recurrent_kernel, const float* recurrent_bias, const float* h0, float* y,
                                    float* saved, void* workspace, size_t workspace_bytes, int batch, int steps, int hidden, void* stream) {
  if (!mx || !recurrent_kernel || !recurrent_bias || !h0 || !y) return DDSP_ERR_NULL_POINTER;
  if (batch < 0 || steps < 1 || hidden < 1) return DDSP_ERR_BAD_SHAPE;
  if (!gru_supported(batch, hidden)) return DDSP_ERR_UNSUPPORTED;
  if (batch == 0) return DDSP_OK;
  const int B = batch, T = steps, H = hidden;
  hipStream_t s = (hipStream_t)stream;
  const bool mfma = H % 16 == 0;
  if (mfma) {
    if (!workspace) return DDSP_ERR_NULL_POINTER;
    if (workspace_bytes < ddsp_gru_forward_workspace_bytes(B, H)) return DDSP_ERR_WORKSPACE;
    gru_prepare(recurrent_kernel, static_cast<char*>(workspace), H, 0, s);
  }
  const u32x4* packed = mfma ? reinterpret_cast<const u32x4*>(static_cast<char*>(workspace) + kHeaderBytes) : nullptr;
  const int* exponent = static_cast<const int*>(workspace);
  const unsigned plain_grid = (unsigned)(((size_t)B * H + 255) / 256);
  for (int t = 0; t < T; ++t) {
    const float* h_prev = t == 0 ? h0 : y + (size_t)(t - 1) * H;
    const size_t h_stride = t == 0 ? (size_t)H : (size_t)T * H;
    if (mfma)
      hipLaunchKernelGGL(gru_fwd_mfma_kernel, dim3(H / 16), dim3(256), 0, s, mx, packed, exponent, recurrent_bias, h_prev, h_stride, y, saved, B,
                         T, H, t);
    else
      hipLaunchKernelGGL(gru_fwd_plain_kernel, dim3(plain_grid), dim3(256), 0, s, mx, recurrent_kernel, recurrent_bias, h_prev, h_stride, y,
                         saved, B, T, H, t);
  }
  return check_launch();
}

extern "C" size_t ddsp_gru_backward_workspace_bytes(int batch, int hidden) {
  if (batch < 1 || hidden < 1 || !gru_supported(batch, hidden)) return 0;
  return kHeaderBytes + packed_bytes(hidden) + 2 * (size_t)batch * hidden * sizeof(float);
}

extern "C" int ddsp_gru_backward_f32(const float* dy, const float* y, const float* h0, const float* saved, const float* recurrent_kernel,
                                     float* d_in, float* d_rec, float* dh0, void* workspace, size_t workspace_bytes, int batch, int steps,
                                     int hidden, void* stream) {
  if (!dy || !y || !h0 || !saved || !recurrent_kernel || !d_in || !d_rec || !dh0) return DDSP_ERR_NULL_POINTER;
  if (batch < 0 || steps < 1 || hidden < 1) return DDSP_ERR_BAD_SHAPE;
  if (!gru_supported(batch, hidden)) return DDSP_ERR_UNSUPPORTED;
  if (batch == 0) return DDSP_OK;
  if (!workspace) return DDSP_ERR_NULL_POINTER;
  if (workspace_bytes < ddsp_gru_backward_workspace_bytes(batch, hidden)) return DDSP_ERR_WORKSPACE;
  const int B = batch, T = steps, H = hidden;
  hipStream_t s = (hipStream_t)stream;
  const bool mfma = H % 16 == 0;
  char* ws = static_cast<char*>(workspace);
  if (mfma) gru_prepare(recurrent_kernel, ws, H, 1, s);
  const u32x4* packed = reinterpret_cast<const u32x4*>(ws + kHeaderBytes);
  const int* exponent = reinterpret_cast<const int*>(ws);
  float* carry[2];
  carry[0] = reinterpret_cast<float*>(ws + kHeaderBytes + packed_bytes(H));
  carry[1] = carry[0] + (size_t)B * H;
  const unsigned plain_grid = (unsigned)(((size_t)B * H + 255) / 256);
  hipLaunchKernelGGL(gru_bwd_init_kernel, dim3(plain_grid), dim3(256), 0, s, dy, carry[0], B, T, H);
  int cur = 0;
  for (int t = T - 1; t >= 0; --t) {
    const float* h_prev = t == 0 ? h0 : y + (size_t)(t - 1) * H;
    const size_t h_stride = t == 0 ? (size_t)H : (size_t)T * H;
    const float* dy_prev = t == 0 ? nullptr : dy + (size_t)(t - 1) * H;
    float* out = t == 0 ? dh0 : carry[cur ^ 1];
    if (mfma)
      hipLaunchKernelGGL(gru_bwd_mfma_kernel, dim3(H / 16), dim3(256), 0, s, carry[cur], saved, packed, exponent, h_prev, h_stride, dy_prev,
                         (size_t)T * H, d_in, d_rec, out, B, T, H, t);
    else
      hipLaunchKernelGGL(gru_bwd_plain_kernel, dim3(plain_grid), dim3(256), 0, s, carry[cur], saved, recurrent_kernel, h_prev, h_stride, dy_prev,
                         (size_t)T * H, d_in, d_rec, out, B, T, H, t);
    cur ^= 1;
  }
  return check_launch();
}
