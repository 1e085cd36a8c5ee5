// The layer ddsp/training/nn.py DilatedConvStack consists of, for gfx950 (C ABI: conv_abi.h): ReLU -> dilated 1-D convolution
// (Conv2D((k, 1), dilation_rate=(d, 1), padding='same')) of a channel-last [batch, time, ch] tensor, and its adjoint in x.
//
//   y[b, t, co] = addend + mask * (bias[co] + sum_k sum_ci act(x[b, t + k d - pad_left, ci]) Wk[k][ci][co])
//
// No padded copy, no im2col: a tap is a row offset, rows outside [0, time) are zeros in the fragment.
//
//   conv_mfma_kernel    ch_out a multiple of 16: the matrix-core product conv_mfma.h describes (its power-of-two scales, its
//                       workspace) over 64 time rows of one batch row.  A step is a (tap, 32-deep slice of ch_in): each wavefront
//                       loads its 16 rows of x for the tap, 32 bytes per lane.  The taps' rows overlap between steps and between
//                       neighbouring blocks, so x comes from HBM once and from cache afterwards.  Taps that lie wholly in the
//                       padding for the block are skipped.
//   conv_pack_kernel    W (or the adjoint's taps: reversed and transposed) as MFMA B fragments, fp16 hi / lo behind 2^-e, once per
//                       call; ch_in tails are zeros.
//   conv_plain_kernel   the vector-ALU form for every other ch_out: a thread per output element, taps and channels in order.
//
// No atomics, every sum in a fixed order, no host synchronisation, the workspace is the caller's: capturable, and the same bits on
// every run, for a row alone and for any sub-batch.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "conv_abi.h"
#include "conv_mfma.h"

namespace ddsp {
namespace conv {

using namespace conv_mfma;

// tap k of the convolution that is computed: [ci][co]
__device__ __forceinline__ float tap_weight(const float* __restrict__ w, int k, int ci, int co, int Cin, int Cout, int K, int transposed) {
  return transposed ? w[((size_t)(K - 1 - k) * Cout + co) * Cin + ci] : w[((size_t)k * Cin + ci) * Cout + co];
}

// MFMA B fragments, scaled by 2^-e, as fp16 hi / lo: fragment (k, ks, ct), part p at u32x4 index
// ((((k KS + ks) CT + ct) 2 + p) 64 + lane; lane l, element q holds B[kk][j] = Wk[k][ks 32 + kk][ct 16 + j], kk = 8 (l / 16) + q,
// j = l % 16, and 0 where ks 32 + kk >= ch_in.  The column tiles of one (tap, step) lie side by side: a block stages a run of them.
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ w, const float* __restrict__ partials, int* __restrict__ exponent,
                                                        u32x4* __restrict__ packed, int Cin, int Cout, int K, int transposed, int n_partials) {
  const int CT = Cout / 16, KS = (Cin + 31) / 32;
  float m = 0.0f;
  for (int i = 0; i < n_partials; ++i) m = fmaxf(m, partials[i]);
  const int e = pow2_exponent(m);
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id == 0) *exponent = e;
  const size_t frag_id = id >> 6;
  if (frag_id >= (size_t)K * KS * CT) return;
  const int lane = (int)(id & 63);
  const int ct = (int)(frag_id % CT), ks = (int)((frag_id / CT) % KS), k = (int)(frag_id / ((size_t)CT * KS));
  const int co = ct * 16 + (lane & 15), c0 = ks * 32 + 8 * (lane >> 4);
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = c0 + q < Cin ? ldexpf(tap_weight(w, k, c0 + q, co, Cin, Cout, K, transposed), -e) : 0.0f;
  store_fragment(packed, frag_id, lane, v);
}

// grid (batch * tiles, column chunks)
__global__ __launch_bounds__(256) void conv_mfma_kernel(const float* __restrict__ x, const u32x4* __restrict__ packed,
                                                        const int* __restrict__ w_exponent, const float* __restrict__ row_partials,
                                                        const float* __restrict__ bias, const float* __restrict__ addend,
                                                        const float* __restrict__ mask_src, float* __restrict__ y, int T, int Cin, int Cout,
                                                        int K, int dilation, int pad_left, int relu, int tiles, int per_row) {
  __shared__ u32x4 stage[2][kChunkTiles * 128];          // the fragments of this block's column tiles for two (tap, step)s: 32 KB
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t b = blockIdx.x / (unsigned)tiles;
  const long long block_t0 = (long long)(blockIdx.x % (unsigned)tiles) * kTilePositions;
  const int CT = Cout / 16, KS = (Cin + 31) / 32;
  const int ct0 = blockIdx.y * kChunkTiles;
  const int nct = CT - ct0 < kChunkTiles ? CT - ct0 : kChunkTiles;
  float m = 0.0f;
  for (int i = 0; i < per_row; ++i) m = fmaxf(m, row_partials[b * per_row + i]);
  const int e_x = pow2_exponent(m);                      // per BATCH ROW
  const long long a_row = block_t0 + wave * 16 + (lane & 15);
  const int c_lane = 8 * (lane >> 4);
  const float* xb = x + b * (size_t)T * Cin;
  // the taps that reach this block's rows are a run k_lo .. k_hi (the shift grows with k); the others are padding here: block-uniform
  int k_lo = K, k_hi = -1;
  for (int k = 0; k < K; ++k) {
    const long long shift = (long long)k * dilation - pad_left;
    if (block_t0 + shift < T && block_t0 + (kTilePositions - 1) + shift >= 0) {
      k_lo = k < k_lo ? k : k_lo;
      k_hi = k;
    }
  }
  const int steps = k_hi < k_lo ? 0 : (k_hi - k_lo + 1) * KS;
  // Step s = (tap k_lo + s / KS, 32-deep slice s % KS).  Its weight fragments and this lane's 8 values of x are fetched into
  // registers one step ahead, while the matrix cores work on the step before; the fragments then go to the stage that step s - 2 used.
  u32x4 b_next[kStageLoads];
  float v_next[8];
  auto fetch = [&](int step) {
    const int k = k_lo + step / KS, ks = step % KS;
    const u32x4* src = packed + (((size_t)k * KS + ks) * CT + ct0) * 128;
#pragma unroll
    for (int i = 0; i < kStageLoads; ++i) {
      const int at = (int)threadIdx.x + 256 * i;
      if (at < nct * 128) b_next[i] = src[at];
    }
    const long long src_row = a_row + (long long)k * dilation - pad_left;
    const int c = ks * 32 + c_lane;
#pragma unroll
    for (int q = 0; q < 8; ++q) v_next[q] = 0.0f;
    if (a_row < T && src_row >= 0 && src_row < T && c < Cin) {
      const float* p = xb + (size_t)src_row * Cin + c;
      if (c + 8 <= Cin) {
        const PackedF4 p0 = *reinterpret_cast<const PackedF4*>(p), p1 = *reinterpret_cast<const PackedF4*>(p + 4);
        v_next[0] = p0.x; v_next[1] = p0.y; v_next[2] = p0.z; v_next[3] = p0.w;
        v_next[4] = p1.x; v_next[5] = p1.y; v_next[6] = p1.z; v_next[7] = p1.w;
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (c + q < Cin) v_next[q] = p[q];
      }
    }
  };
  f32x4 acc[kChunkTiles], cross[kChunkTiles];
#pragma unroll
  for (int j = 0; j < kChunkTiles; ++j) acc[j] = cross[j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  if (steps) fetch(0);
  for (int step = 0; step < steps; ++step) {
    u32x4* buf = stage[step & 1];                        // its readers of step - 2 are behind the barrier of step - 1
#pragma unroll
    for (int i = 0; i < kStageLoads; ++i) {
      const int at = (int)threadIdx.x + 256 * i;
      if (at < nct * 128) buf[at] = b_next[i];
    }
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = ldexpf(relu ? relu_keep_nan(v_next[q]) : v_next[q], -e_x);
    f16x8 a_hi, a_lo;
    split8(v, a_hi, a_lo);
    __syncthreads();
    if (step + 1 < steps) fetch(step + 1);
#pragma unroll
    for (int j = 0; j < kChunkTiles; ++j) {
      if (j < nct) {                                     // block-uniform
        const f16x8 b_hi = __builtin_bit_cast(f16x8, buf[j * 128 + lane]), b_lo = __builtin_bit_cast(f16x8, buf[j * 128 + 64 + lane]);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_hi, acc[j], 0, 0, 0);
        cross[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_lo, cross[j], 0, 0, 0);
        cross[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, b_hi, cross[j], 0, 0, 0);
      }
    }
  }
  const int e = e_x + *w_exponent;
#pragma unroll
  for (int j = 0; j < kChunkTiles; ++j) {
    if (j < nct) {
      const int co = (ct0 + j) * 16 + (lane & 15);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long long row = block_t0 + wave * 16 + 4 * (lane >> 4) + q;
        if (row < T) {
          const size_t at = (b * (size_t)T + (size_t)row) * Cout + co;
          y[at] = epilogue(ldexpf(combine(acc[j][q], cross[j][q]), e), at, co, bias, addend, mask_src);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void conv_plain_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ addend, const float* __restrict__ mask_src,
                                                         float* __restrict__ y, size_t n_out, int T, int Cin, int Cout, int K, int dilation,
                                                         int pad_left, int relu, int transposed) {
  const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= n_out) return;
  const size_t row = at / Cout;
  const int co = (int)(at % Cout);
  const size_t b = row / T;
  const long long t = (long long)(row % T);
  float sum = 0.0f;
  for (int k = 0; k < K; ++k) {
    const long long s = t + (long long)k * dilation - pad_left;
    if (s < 0 || s >= T) continue;
    const float* xr = x + (b * (size_t)T + (size_t)s) * Cin;
    for (int ci = 0; ci < Cin; ++ci) {
      const float a = relu ? relu_keep_nan(xr[ci]) : xr[ci];
      sum = fmaf(a, tap_weight(w, k, ci, co, Cin, Cout, K, transposed), sum);
    }
  }
  y[at] = epilogue(sum, at, co, bias, addend, mask_src);
}

static inline size_t packed_bytes(int ch_in, int ch_out, int taps) {
  return (size_t)taps * ((ch_in + 31) / 32) * (ch_out / 16) * 128 * sizeof(u32x4);
}
static inline bool well_formed(int batch, int time, int ch_in, int ch_out, int taps) {
  return batch >= 0 && time >= 1 && ch_in >= 1 && ch_out >= 1 && taps >= 1;
}
static inline bool supported(int batch, int time, int ch_in, int ch_out, int taps) {
  const int ch = ch_in > ch_out ? ch_in : ch_out;
  return ch <= DDSP_CONVD_MAX_CHANNELS && taps <= DDSP_CONVD_MAX_TAPS && (size_t)batch * (size_t)time * (size_t)ch < ((size_t)1 << 31);
}

}  // namespace conv
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::conv;

extern "C" size_t ddsp_dilated_conv_workspace_bytes(int batch, int time, int ch_in, int ch_out, int taps) {
  if (!well_formed(batch, time, ch_in, ch_out, taps) || batch == 0 || !supported(batch, time, ch_in, ch_out, taps) || ch_out % 16 != 0) return 0;
  return fragments_offset(batch) + packed_bytes(ch_in, ch_out, taps);
}

extern "C" int ddsp_dilated_conv_f32(const float* x, const float* W, const float* bias, const float* addend, const float* mask_src, float* y,
                                     void* workspace, size_t workspace_bytes, int batch, int time, int ch_in, int ch_out, int taps,
                                     int dilation, int pad_left, unsigned flags, void* stream) {
  const unsigned known = DDSP_CONVD_RELU_INPUT | DDSP_CONVD_TRANSPOSE_W | DDSP_CONVD_MASK_OUTPUT;
  if (!x || !W || !y || ((flags & DDSP_CONVD_MASK_OUTPUT) && !mask_src)) return DDSP_ERR_NULL_POINTER;
  if (!well_formed(batch, time, ch_in, ch_out, taps) || dilation < 1 || pad_left < 0 || (flags & ~known)) return DDSP_ERR_BAD_SHAPE;
  if (!supported(batch, time, ch_in, ch_out, taps) || (long long)(taps - 1) * dilation > INT_MAX) return DDSP_ERR_UNSUPPORTED;
  if ((long long)pad_left > (long long)(taps - 1) * dilation) return DDSP_ERR_BAD_SHAPE;
  if (batch == 0) return DDSP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int relu = (flags & DDSP_CONVD_RELU_INPUT) ? 1 : 0, transposed = (flags & DDSP_CONVD_TRANSPOSE_W) ? 1 : 0;
  const float* mask = (flags & DDSP_CONVD_MASK_OUTPUT) ? mask_src : nullptr;
  if (ch_out % 16 != 0) {
    const size_t n_out = (size_t)batch * time * ch_out;
    hipLaunchKernelGGL(conv_plain_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, x, W, bias, addend, mask, y, n_out, time, ch_in,
                       ch_out, taps, dilation, pad_left, relu, transposed);
    return check_launch();
  }
  if (!workspace) return DDSP_ERR_NULL_POINTER;
  if (workspace_bytes < ddsp_dilated_conv_workspace_bytes(batch, time, ch_in, ch_out, taps)) return DDSP_ERR_WORKSPACE;
  const Workspace ws = carve(workspace, batch);
  const Partials p = launch_absmax(ws, W, (size_t)taps * ch_in * ch_out, x, (size_t)time * ch_in, batch, relu, s);
  const size_t pack_threads = (size_t)taps * ((ch_in + 31) / 32) * (ch_out / 16) * 64;
  hipLaunchKernelGGL(conv_pack_kernel, dim3((unsigned)((pack_threads + 255) / 256)), dim3(256), 0, s, W, ws.w_partials, ws.exponent, ws.packed, ch_in,
                     ch_out, taps, transposed, p.w_blocks);
  const int tiles = (time + kTilePositions - 1) / kTilePositions;
  const dim3 grid((unsigned)((size_t)batch * tiles), (unsigned)((ch_out / 16 + kChunkTiles - 1) / kChunkTiles));
  hipLaunchKernelGGL(conv_mfma_kernel, grid, dim3(256), 0, s, x, ws.packed, ws.exponent, ws.row_partials, bias, addend, mask, y, time, ch_in, ch_out,
                     taps, dilation, pad_left, relu, tiles, p.per_row);
  return check_launch();
}
