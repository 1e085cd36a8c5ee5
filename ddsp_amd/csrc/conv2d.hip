// The convolution ddsp/training/nn.py's ResNet consists of, for gfx950 (C ABI: conv2d_abi.h): (ReLU ->) Conv2D(ch, (kh, kw),
// (sh, sw), padding='same') of a channel-last [batch, h, w, ch] tensor, and its adjoint in x.  The 2-D sibling of dilated_conv.hip.
//
//   y[b, oh, ow, co] = addend + mask * (bias[co] + sum_{i, j, ci} act(x[b, oh sh + i - top, ow sw + j - left, ci]) W[i][j][ci][co])
//
// No padded copy, no im2col: the product's K axis is the flattened (i, j, ci) - the Keras kernel [kh, kw, ci, co] read as a
// [kh kw ci, co] matrix - and a K index maps to a source position per lane; positions outside the image are zeros in the fragment.
// Forward and adjoint are ONE kernel: they differ in source_position() (output position, tap -> source position or none: the
// adjoint gathers the gradient at (r + top - i) / sh where the division is exact) and in how conv2d_pack_kernel reads W.
//
//   conv2d_mfma_kernel    produced width a multiple of 16: the matrix-core product conv_mfma.h describes (its power-of-two
//                         scales, its workspace) over a run of 64 output positions of one batch row; the run is over the flattened
//                         (oh, ow), so it crosses image rows where out_w is small and each lane resolves its own position.  A step
//                         is 32 K rows: each lane loads its 8 K values of its position - with the source width a multiple of 8
//                         they are 32 contiguous bytes of one tap, otherwise (the stem: one channel, 49 taps in two steps) eight
//                         positions.
//   conv2d_pack_kernel    W as MFMA B fragments over the flattened K axis, fp16 hi / lo behind 2^-e, once per call; the K tail is 0.
//   conv2d_plain_kernel   the vector-ALU form for every other width: a thread per output element, taps and channels in order.
//
// No atomics, every sum in a fixed order, no host synchronisation, the workspace is the caller's: capturable, and the same bits on
// every run, for a row alone and for any sub-batch.  No value of x reaches an index.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "conv2d_abi.h"
#include "conv_mfma.h"

namespace ddsp {
namespace conv2d {

using namespace conv_mfma;

// The call as the kernels see it: `src` is what is read (x forward, the gradient in the adjoint), `dst` what is written.
struct Geometry {
  int src_h, src_w, src_ch;
  int dst_h, dst_w, dst_ch;
  int kh, kw, sh, sw, top, left;
  int adjoint;
};

// The position (row * src_w + column) that destination (r, c) reads under tap (i, j), or -1 where there is none: the only thing in
// which the convolution and its adjoint differ on the activation side.
__device__ __forceinline__ int source_position(const Geometry& g, int r, int c, int i, int j) {
  int sr, sc;
  if (!g.adjoint) {
    sr = r * g.sh + i - g.top;
    sc = c * g.sw + j - g.left;
  } else {
    const int nr = r + g.top - i, nc = c + g.left - j;
    if (nr < 0 || nc < 0) return -1;
    sr = nr / g.sh;
    sc = nc / g.sw;
    if (sr * g.sh != nr || sc * g.sw != nc) return -1;
  }
  if (sr < 0 || sr >= g.src_h || sc < 0 || sc >= g.src_w) return -1;
  return sr * g.src_w + sc;
}

// B[kk][col] of the product: kk = (i kw + j) src_ch + cs over W [kh, kw, ch_in, ch_out]
__device__ __forceinline__ float weight_at(const float* __restrict__ w, const Geometry& g, int tap, int cs, int col) {
  return g.adjoint ? w[((size_t)tap * g.dst_ch + col) * g.src_ch + cs] : w[((size_t)tap * g.src_ch + cs) * g.dst_ch + col];
}

// MFMA B fragments, scaled by 2^-e, as fp16 hi / lo: fragment (ks, ct), part p at u32x4 index ((ks CT + ct) 2 + p) 64 + lane; lane l,
// element q holds B[kk][col], kk = 32 ks + 8 (l / 16) + q, col = 16 ct + l % 16, and 0 where kk >= kh kw src_ch.  The column tiles
// of one step lie side by side: a block stages a run of them.
__global__ __launch_bounds__(256) void conv2d_pack_kernel(const float* __restrict__ w, const float* __restrict__ partials,
                                                          int* __restrict__ exponent, u32x4* __restrict__ packed, Geometry g,
                                                          int n_partials) {
  const int CT = g.dst_ch / 16, KT = g.kh * g.kw * g.src_ch, KS = (KT + 31) / 32;
  float m = 0.0f;
  for (int i = 0; i < n_partials; ++i) m = fmaxf(m, partials[i]);
  const int e = pow2_exponent(m);
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id == 0) *exponent = e;
  const size_t frag_id = id >> 6;
  if (frag_id >= (size_t)KS * CT) return;
  const int lane = (int)(id & 63);
  const int ct = (int)(frag_id % CT), ks = (int)(frag_id / CT);
  const int col = ct * 16 + (lane & 15), k0 = ks * 32 + 8 * (lane >> 4);
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int kk = k0 + q;
    v[q] = kk < KT ? ldexpf(weight_at(w, g, kk / g.src_ch, kk % g.src_ch, col), -e) : 0.0f;
  }
  store_fragment(packed, frag_id, lane, v);
}

// grid (batch * tiles, column chunks)
__global__ __launch_bounds__(256) void conv2d_mfma_kernel(const float* __restrict__ x, const u32x4* __restrict__ packed,
                                                          const int* __restrict__ w_exponent, const float* __restrict__ row_partials,
                                                          const float* __restrict__ bias, const float* __restrict__ addend,
                                                          const float* __restrict__ mask_src, float* __restrict__ y, Geometry g, int relu,
                                                          int tiles, int per_row) {
  __shared__ u32x4 stage[2][kChunkTiles * 128];          // the fragments of this block's column tiles for two steps: 32 KB
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t b = blockIdx.x / (unsigned)tiles;
  const long long block_p0 = (long long)(blockIdx.x % (unsigned)tiles) * kTilePositions;
  const long long positions = (long long)g.dst_h * g.dst_w;
  const int CT = g.dst_ch / 16, KT = g.kh * g.kw * g.src_ch, steps = (KT + 31) / 32;
  const int ct0 = blockIdx.y * kChunkTiles;
  const int nct = CT - ct0 < kChunkTiles ? CT - ct0 : kChunkTiles;
  const bool one_tap = g.src_ch % 8 == 0;                // a lane's 8 K values are 32 contiguous bytes of one tap: the fast path
  float m = 0.0f;
  for (int i = 0; i < per_row; ++i) m = fmaxf(m, row_partials[b * per_row + i]);
  const int e_x = pow2_exponent(m);                      // per BATCH ROW
  // this lane's row of the A fragment: one output position, resolved per lane (a run of 64 crosses image rows)
  const long long a_pos = block_p0 + wave * 16 + (lane & 15);
  const bool a_live = a_pos < positions;
  const int a_r = a_live ? (int)(a_pos / g.dst_w) : 0, a_c = a_live ? (int)(a_pos % g.dst_w) : 0;
  const int k_lane = 8 * (lane >> 4);
  const float* xb = x + b * (size_t)g.src_h * g.src_w * g.src_ch;
  // Step s is K rows 32 s .. 32 s + 31.  Its weight fragments and this lane's 8 values of x are fetched into registers one step
  // ahead, while the matrix cores work on the step before; the fragments then go to the stage that step s - 2 used.
  u32x4 b_next[kStageLoads];
  float v_next[8];
  auto fetch = [&](int step) {
    const u32x4* src = packed + ((size_t)step * CT + ct0) * 128;
#pragma unroll
    for (int i = 0; i < kStageLoads; ++i) {
      const int at = (int)threadIdx.x + 256 * i;
      if (at < nct * 128) b_next[i] = src[at];
    }
    const int k0 = step * 32 + k_lane;
#pragma unroll
    for (int q = 0; q < 8; ++q) v_next[q] = 0.0f;
    if (!a_live || k0 >= KT) return;
    if (one_tap) {
      const int tap = k0 / g.src_ch, cs = k0 - tap * g.src_ch, i = tap / g.kw;
      const int pos = source_position(g, a_r, a_c, i, tap - i * g.kw);
      if (pos >= 0) {
        const float* p = xb + (size_t)pos * g.src_ch + cs;
        const PackedF4 p0 = *reinterpret_cast<const PackedF4*>(p), p1 = *reinterpret_cast<const PackedF4*>(p + 4);
        v_next[0] = p0.x; v_next[1] = p0.y; v_next[2] = p0.z; v_next[3] = p0.w;
        v_next[4] = p1.x; v_next[5] = p1.y; v_next[6] = p1.z; v_next[7] = p1.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int kk = k0 + q;
        if (kk < KT) {
          const int tap = kk / g.src_ch, cs = kk - tap * g.src_ch, i = tap / g.kw;
          const int pos = source_position(g, a_r, a_c, i, tap - i * g.kw);
          if (pos >= 0) v_next[q] = xb[(size_t)pos * g.src_ch + cs];
        }
      }
    }
  };
  f32x4 acc[kChunkTiles], cross[kChunkTiles];
#pragma unroll
  for (int j = 0; j < kChunkTiles; ++j) acc[j] = cross[j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  fetch(0);
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
      const int col = (ct0 + j) * 16 + (lane & 15);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long long pos = block_p0 + wave * 16 + 4 * (lane >> 4) + q;
        if (pos < positions) {
          const size_t at = (b * (size_t)positions + (size_t)pos) * g.dst_ch + col;
          y[at] = epilogue(ldexpf(combine(acc[j][q], cross[j][q]), e), at, col, bias, addend, mask_src);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void conv2d_plain_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, const float* __restrict__ addend,
                                                           const float* __restrict__ mask_src, float* __restrict__ y, size_t n_out,
                                                           Geometry g, int relu) {
  const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= n_out) return;
  const size_t positions = (size_t)g.dst_h * g.dst_w;
  const size_t flat = at / g.dst_ch;
  const int col = (int)(at % g.dst_ch);
  const size_t b = flat / positions;
  const size_t pos = flat % positions;
  const int r = (int)(pos / g.dst_w), c = (int)(pos % g.dst_w);
  const float* xb = x + b * (size_t)g.src_h * g.src_w * g.src_ch;
  float sum = 0.0f;
  for (int i = 0; i < g.kh; ++i) {
    for (int j = 0; j < g.kw; ++j) {
      const int s = source_position(g, r, c, i, j);
      if (s < 0) continue;
      const float* xr = xb + (size_t)s * g.src_ch;
      for (int cs = 0; cs < g.src_ch; ++cs) {
        const float a = relu ? relu_keep_nan(xr[cs]) : xr[cs];
        sum = fmaf(a, weight_at(w, g, i * g.kw + j, cs, col), sum);
      }
    }
  }
  y[at] = epilogue(sum, at, col, bias, addend, mask_src);
}

static inline size_t packed_bytes(int src_ch, int dst_ch, int taps) {
  return (((size_t)taps * src_ch + 31) / 32) * (dst_ch / 16) * 128 * sizeof(u32x4);
}
static inline bool well_formed(int batch, int h, int w, int ch_in, int ch_out, int kh, int kw, int sh, int sw) {
  return batch >= 0 && h >= 1 && w >= 1 && ch_in >= 1 && ch_out >= 1 && kh >= 1 && kw >= 1 && sh >= 1 && sw >= 1;
}
// TF 'same': the output size along an axis and the padding in front of it
static inline int out_size(int n, int stride) { return (int)(((long long)n + stride - 1) / stride); }
static inline int pad_before(int n, int k, int stride) {
  const long long total = (long long)(out_size(n, stride) - 1) * stride + k - n;
  return (int)((total > 0 ? total : 0) / 2);
}
static inline bool supported(int batch, int h, int w, int ch_in, int ch_out, int kh, int kw, int sh, int sw) {
  const size_t limit = (size_t)1 << 31;
  if (ch_in > DDSP_CONV2D_MAX_CHANNELS || ch_out > DDSP_CONV2D_MAX_CHANNELS || (long long)kh * kw > DDSP_CONV2D_MAX_TAPS) return false;
  if (sh > DDSP_CONV2D_MAX_STRIDE || sw > DDSP_CONV2D_MAX_STRIDE || h > (1 << 30) || w > (1 << 30)) return false;
  const size_t in_positions = (size_t)h * (size_t)w, out_positions = (size_t)out_size(h, sh) * (size_t)out_size(w, sw);
  if (in_positions >= limit || out_positions >= limit) return false;
  return (size_t)batch * in_positions * ch_in < limit && (size_t)batch * out_positions * ch_out < limit;
}
static inline Geometry geometry(int h, int w, int ch_in, int ch_out, int kh, int kw, int sh, int sw, int adjoint) {
  const int out_h = out_size(h, sh), out_w = out_size(w, sw);
  Geometry g;
  g.src_h = adjoint ? out_h : h, g.src_w = adjoint ? out_w : w, g.src_ch = adjoint ? ch_out : ch_in;
  g.dst_h = adjoint ? h : out_h, g.dst_w = adjoint ? w : out_w, g.dst_ch = adjoint ? ch_in : ch_out;
  g.kh = kh, g.kw = kw, g.sh = sh, g.sw = sw, g.top = pad_before(h, kh, sh), g.left = pad_before(w, kw, sw);
  g.adjoint = adjoint;
  return g;
}

}  // namespace conv2d
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::conv2d;

extern "C" size_t ddsp_conv2d_workspace_bytes(int batch, int h, int w, int ch_in, int ch_out, int kh, int kw, int sh, int sw, unsigned flags) {
  if (!well_formed(batch, h, w, ch_in, ch_out, kh, kw, sh, sw) || batch == 0 || !supported(batch, h, w, ch_in, ch_out, kh, kw, sh, sw)) return 0;
  const int adjoint = (flags & DDSP_CONV2D_ADJOINT) ? 1 : 0;
  const int src_ch = adjoint ? ch_out : ch_in, dst_ch = adjoint ? ch_in : ch_out;
  if (dst_ch % 16 != 0) return 0;
  return fragments_offset(batch) + packed_bytes(src_ch, dst_ch, kh * kw);
}

extern "C" int ddsp_conv2d_f32(const float* x, const float* W, const float* bias, const float* addend, const float* mask_src, float* y,
                               void* workspace, size_t workspace_bytes, int batch, int h, int w, int ch_in, int ch_out, int kh, int kw,
                               int sh, int sw, unsigned flags, void* stream) {
  const unsigned known = DDSP_CONV2D_RELU_INPUT | DDSP_CONV2D_ADJOINT | DDSP_CONV2D_MASK_OUTPUT;
  if (!x || !W || !y || ((flags & DDSP_CONV2D_MASK_OUTPUT) && !mask_src)) return DDSP_ERR_NULL_POINTER;
  if (!well_formed(batch, h, w, ch_in, ch_out, kh, kw, sh, sw) || (flags & ~known)) return DDSP_ERR_BAD_SHAPE;
  if (!supported(batch, h, w, ch_in, ch_out, kh, kw, sh, sw)) return DDSP_ERR_UNSUPPORTED;
  if (batch == 0) return DDSP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int relu = (flags & DDSP_CONV2D_RELU_INPUT) ? 1 : 0;
  const float* mask = (flags & DDSP_CONV2D_MASK_OUTPUT) ? mask_src : nullptr;
  const Geometry g = geometry(h, w, ch_in, ch_out, kh, kw, sh, sw, (flags & DDSP_CONV2D_ADJOINT) ? 1 : 0);
  const size_t positions = (size_t)g.dst_h * g.dst_w;
  if (g.dst_ch % 16 != 0) {
    const size_t n_out = (size_t)batch * positions * g.dst_ch;
    hipLaunchKernelGGL(conv2d_plain_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, x, W, bias, addend, mask, y, n_out, g, relu);
    return check_launch();
  }
  if (!workspace) return DDSP_ERR_NULL_POINTER;
  if (workspace_bytes < ddsp_conv2d_workspace_bytes(batch, h, w, ch_in, ch_out, kh, kw, sh, sw, flags)) return DDSP_ERR_WORKSPACE;
  const Workspace ws = carve(workspace, batch);
  const Partials p = launch_absmax(ws, W, (size_t)kh * kw * ch_in * ch_out, x, (size_t)g.src_h * g.src_w * g.src_ch, batch, relu, s);
  const size_t pack_threads = (((size_t)kh * kw * g.src_ch + 31) / 32) * (g.dst_ch / 16) * 64;
  hipLaunchKernelGGL(conv2d_pack_kernel, dim3((unsigned)((pack_threads + 255) / 256)), dim3(256), 0, s, W, ws.w_partials, ws.exponent, ws.packed, g,
                     p.w_blocks);
  const int tiles = (int)((positions + kTilePositions - 1) / kTilePositions);
  const dim3 grid((unsigned)((size_t)batch * tiles), (unsigned)((g.dst_ch / 16 + kChunkTiles - 1) / kChunkTiles));
  hipLaunchKernelGGL(conv2d_mfma_kernel, grid, dim3(256), 0, s, x, ws.packed, ws.exponent, ws.row_partials, bias, addend, mask, y, g, relu, tiles,
                     p.per_row);
  return check_launch();
}
