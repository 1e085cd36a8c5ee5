// Instance / layer / group normalisation of a channel-last tensor for gfx950 (C ABI: norm_abi.h): what ddsp/training/nn.py
// normalize_op does with a reshape, tf.nn.moments over (h, w, channels of the group), a subtract and a divide, and what
// Normalize adds to it (scale, shift) - one kernel each way while a batch row's slab is one block's work, three or four small
// launches beyond.  x is [N, S, C], S = h * w; group g holds the D = C / G adjacent channels g D .. (g + 1) D - 1.
//
//   LANES.  A block walks the flat [rows * C] memory of its batch row.  For C <= 256 its ACTIVE thread count is the largest
//   multiple of C not above 256, thread t sits on channel t % C and takes rows t / C, t / C + R, ... (R = 256 / C): consecutive
//   lanes read consecutive addresses whatever C is, and a thread never changes its channel, so its sums are one channel's.
//   For C > 256 the 256 lanes lie across a tile of 256 channels and loop over the rows, tile after tile.
//
//   MOMENTS.  Never E[x^2] - mean^2.  Each (chunk of rows, channel) gets its own mean and M2 = sum (x - mean)^2 in two passes
//   over the chunk (at most kChunkElems floats: the second pass and the normalisation re-read it from L2); a group's moments are
//   the fixed-order merge of its K * D chunk-channels: mean = sum cnt_i mean_i / cnt, M2 = sum (M2_i + cnt_i (mean_i - mean)^2).
//   A channel of equal values has mean = that value exactly (min == max), and so has a group of equal chunk-channel means:
//   a constant group has variance 0, xhat = 0, and rstd = 1 / sqrt(eps).
//
//   SPLIT.  While one chunk covers the batch row (S * C <= kChunkElems) and C <= kFusedMaxC, ONE block per batch row does
//   everything: channel moments to LDS, group moments, normalise (gn_fwd_fused_kernel, gn_bwd_fused_kernel).  Beyond, a batch
//   row is K chunks = K blocks: gn_chunk_moments_kernel writes the chunk-channel (mean, M2) to the workspace,
//   gn_group_moments_kernel merges them (a thread, a wavefront or a block per (batch row, group)), gn_apply_kernel normalises; the
//   backward likewise with the sums of dy and dy xhat.  The launch boundary is the only synchronisation: nothing polls memory.
//
//   PARAMETER GRADIENTS.  dshift[c] = sum dy, dscale[c] = sum dy xhat: the per-(batch row, chunk) channel sums the backward needs
//   anyway are kept as partial rows in the workspace and summed in ascending order by gn_param_reduce_kernel.
//
// No atomics; every sum has a fixed order that depends on (S, C, G) alone: the same bits on every run, and a batch row alone
// gives the bits it has inside a batch (dscale / dshift sum over the batch and depend on its size, as any batch sum does).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "norm_abi.h"
#include "common.h"
#include "launch.h"

namespace ddsp {
namespace norm {

constexpr int kThreads = 256;
constexpr int kChunkElems = 16384;         // floats of a batch row one block takes (64 KiB): above, the row is split
constexpr int kFusedMaxC = 2048;           // channels whose moments the one-block kernels keep in LDS
constexpr int kSerialEntries = 8;          // chunk-channels per group up to which ONE thread merges them (a wavefront beyond)
constexpr int kBlockEntries = 1024;        // ... from which a whole block does (split path only: a wavefront alone waits on 16+ loads in turn)

struct Geo {
  int S, C, G, D;
  int TW, R, tiles;      // lanes across TW channels, R row lanes (TW * R active threads), channel tiles
  int rpc, K;            // rows per chunk, chunks per batch row
  float eps;
};

struct Scratch { float a[kThreads], b[kThreads], c[kThreads], bc[kThreads]; };

__device__ __forceinline__ int rows_of(const Geo& p, int k) { return min(p.rpc, p.S - k * p.rpc); }

// who merges a group's chunk-channels: one thread, the 64 lanes of a wavefront, or the four wavefronts of a block
enum { kByThread = 0, kByWave = 1, kByBlock = 2 };
__device__ __forceinline__ int merge_mode(int entries) {
  return entries <= kSerialEntries ? kByThread : (entries < kBlockEntries ? kByWave : kByBlock);
}
enum { kSum = 0, kMin = 1, kMax = 2 };
// the callers' values reduced in a fixed order, result in every caller: the wavefront's butterfly, then (kByBlock; the whole block
// calls) the four wavefronts' results in ascending order through `lds` (kThreads / 64 floats)
template <int OP>
__device__ __forceinline__ float merge(float v, int mode, float* lds) {
  if (mode == kByThread) return v;
  v = OP == kSum ? wave_sum(v) : (OP == kMin ? wave_min(v) : wave_max(v));
  if (mode == kByWave) return v;
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = lds[0];
  for (int w = 1; w < kThreads / 64; ++w) r = OP == kSum ? r + lds[w] : (OP == kMin ? fminf(r, lds[w]) : fmaxf(r, lds[w]));
  __syncthreads();
  return r;
}

// (mean, M2) of every channel over rows [row_lo, row_hi) of one batch row, two passes: ch[c] = mean, ch[C + c] = M2.
// Called by the whole block; ends behind a barrier.
__device__ __forceinline__ void channel_moments(const float* __restrict__ xb, int row_lo, int row_hi, const Geo& p, float* ch,
                                                Scratch& sc) {
  const int t = threadIdx.x, cl = t % p.TW, r0 = t / p.TW;
  const bool on = t < p.TW * p.R;
  const float inv = 1.0f / (float)(row_hi - row_lo);
  for (int tile = 0; tile < p.tiles; ++tile) {
    const int c = tile * p.TW + cl;
    const bool live = on && c < p.C;
    float s = 0.0f, lo = INFINITY, hi = -INFINITY;
    if (live) {
      for (int row = row_lo + r0; row < row_hi; row += p.R) {
        const float v = xb[row * p.C + c];
        s += v; lo = fminf(lo, v); hi = fmaxf(hi, v);
      }
    }
    sc.a[t] = s; sc.b[t] = lo; sc.c[t] = hi;
    __syncthreads();
    if (t < p.TW) {
      float tot = 0.0f, l = INFINITY, h = -INFINITY;
      for (int j = 0; j < p.R; ++j) {
        tot += sc.a[cl + j * p.TW]; l = fminf(l, sc.b[cl + j * p.TW]); h = fmaxf(h, sc.c[cl + j * p.TW]);
      }
      sc.bc[cl] = l == h ? l : tot * inv;
    }
    __syncthreads();
    const float m = sc.bc[cl];
    float q = 0.0f;
    if (live) {
      for (int row = row_lo + r0; row < row_hi; row += p.R) {
        const float d = xb[row * p.C + c] - m;
        q = fmaf(d, d, q);
      }
    }
    sc.a[t] = q;
    __syncthreads();
    if (t < p.TW && c < p.C) {
      float tot = 0.0f;
      for (int j = 0; j < p.R; ++j) tot += sc.a[cl + j * p.TW];
      ch[c] = m;
      ch[p.C + c] = tot;
    }
    __syncthreads();
  }
}

// The mean and rstd of group g, merged from the (mean, M2) of its K * D chunk-channels (chunk k at ch + k * k_stride) in the
// order start, start + step, ... by each caller, the callers' shares merged as `mode` says (merge()).
__device__ __forceinline__ void group_moments(const float* ch, int k_stride, int g, const Geo& p, int start, int step, int mode,
                                              float* lds, float& mean, float& rstd) {
  const int entries = p.K * p.D;
  const float total = (float)p.S * (float)p.D;
  float s = 0.0f, lo = INFINITY, hi = -INFINITY;
  for (int e = start; e < entries; e += step) {
    const int k = e / p.D, j = e - k * p.D;
    const float m = ch[(size_t)k * k_stride + g * p.D + j];
    s = fmaf((float)rows_of(p, k), m, s); lo = fminf(lo, m); hi = fmaxf(hi, m);
  }
  s = merge<kSum>(s, mode, lds); lo = merge<kMin>(lo, mode, lds); hi = merge<kMax>(hi, mode, lds);
  mean = lo == hi ? lo : s / total;
  float q = 0.0f;
  for (int e = start; e < entries; e += step) {
    const int k = e / p.D, j = e - k * p.D;
    const float* at = ch + (size_t)k * k_stride + g * p.D + j;
    const float d = at[0] - mean;
    q += fmaf((float)rows_of(p, k) * d, d, at[p.C]);
  }
  q = merge<kSum>(q, mode, lds);
  rstd = 1.0f / sqrtf(q / total + p.eps);
}

// y = xhat * scale + shift (or xhat) over rows [row_lo, row_hi); gm, gr: the batch row's group means and rstds
__device__ __forceinline__ void apply_fwd(const float* __restrict__ xb, float* __restrict__ yb, int row_lo, int row_hi, const Geo& p,
                                          const float* gm, const float* gr, const float* __restrict__ scale,
                                          const float* __restrict__ shift) {
  const int t = threadIdx.x, cl = t % p.TW, r0 = t / p.TW;
  if (t >= p.TW * p.R) return;
  for (int tile = 0; tile < p.tiles; ++tile) {
    const int c = tile * p.TW + cl;
    if (c >= p.C) break;
    const int g = c / p.D;
    const float m = gm[g], r = gr[g];
    const float a = scale ? scale[c] : 1.0f, b = scale ? shift[c] : 0.0f;
    for (int row = row_lo + r0; row < row_hi; row += p.R) {
      const float h = (xb[row * p.C + c] - m) * r;
      yb[row * p.C + c] = scale ? fmaf(h, a, b) : h;
    }
  }
}

// part[c] = sum dy, part[C + c] = sum dy xhat over rows [row_lo, row_hi), per channel.  Whole block; ends behind a barrier.
__device__ __forceinline__ void channel_grad_sums(const float* __restrict__ dyb, const float* __restrict__ xb, int row_lo, int row_hi,
                                                  const Geo& p, const float* __restrict__ gm, const float* __restrict__ gr, float* part,
                                                  Scratch& sc) {
  const int t = threadIdx.x, cl = t % p.TW, r0 = t / p.TW;
  const bool on = t < p.TW * p.R;
  for (int tile = 0; tile < p.tiles; ++tile) {
    const int c = tile * p.TW + cl;
    const bool live = on && c < p.C;
    float a = 0.0f, b = 0.0f;
    if (live) {
      const int g = c / p.D;
      const float m = gm[g], r = gr[g];
      for (int row = row_lo + r0; row < row_hi; row += p.R) {
        const float d = dyb[row * p.C + c];
        a += d;
        b = fmaf(d, (xb[row * p.C + c] - m) * r, b);
      }
    }
    sc.a[t] = a; sc.b[t] = b;
    __syncthreads();
    if (t < p.TW && c < p.C) {
      float ta = 0.0f, tb = 0.0f;
      for (int j = 0; j < p.R; ++j) { ta += sc.a[cl + j * p.TW]; tb += sc.b[cl + j * p.TW]; }
      part[c] = ta;
      part[p.C + c] = tb;
    }
    __syncthreads();
  }
}

// mean over group g of g' = dy scale and of g' xhat, from the channel sums of its K * D chunk-channels (order as group_moments)
__device__ __forceinline__ void group_grad_means(const float* part, int k_stride, int g, const Geo& p, const float* __restrict__ scale,
                                                 int start, int step, int mode, float* lds, float& ga, float& gb) {
  const int entries = p.K * p.D;
  float a = 0.0f, b = 0.0f;
  for (int e = start; e < entries; e += step) {
    const int k = e / p.D, c = g * p.D + (e - k * p.D);
    const float* at = part + (size_t)k * k_stride + c;
    const float w = scale ? scale[c] : 1.0f;
    a = fmaf(w, at[0], a);
    b = fmaf(w, at[p.C], b);
  }
  a = merge<kSum>(a, mode, lds); b = merge<kSum>(b, mode, lds);
  const float total = (float)p.S * (float)p.D;
  ga = a / total;
  gb = b / total;
}

// dx = rstd ((g' - mean(g')) - xhat mean(g' xhat)) over rows [row_lo, row_hi); ga, gb: the batch row's group means
__device__ __forceinline__ void apply_bwd(const float* __restrict__ dyb, const float* __restrict__ xb, float* __restrict__ dxb, int row_lo,
                                          int row_hi, const Geo& p, const float* __restrict__ gm, const float* __restrict__ gr,
                                          const float* ga, const float* gb, const float* __restrict__ scale) {
  const int t = threadIdx.x, cl = t % p.TW, r0 = t / p.TW;
  if (t >= p.TW * p.R) return;
  for (int tile = 0; tile < p.tiles; ++tile) {
    const int c = tile * p.TW + cl;
    if (c >= p.C) break;
    const int g = c / p.D;
    const float m = gm[g], r = gr[g], s1 = ga[g], s2 = gb[g];
    const float w = scale ? scale[c] : 1.0f;
    for (int row = row_lo + r0; row < row_hi; row += p.R) {
      const float h = (xb[row * p.C + c] - m) * r;
      // the product is rounded on its own (no FMA with - s1): a one-element group then has g' - mean(g') = 0 exactly
      dxb[row * p.C + c] = r * ((rn_mul(dyb[row * p.C + c], w) - s1) - h * s2);
    }
  }
}

// ---- one block per batch row -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gn_fwd_fused_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, float* __restrict__ y,
                                                                float* __restrict__ mean_out, float* __restrict__ rstd_out, Geo p) {
  __shared__ Scratch sc;
  __shared__ float ch[2 * kFusedMaxC];
  __shared__ float gs[2 * kFusedMaxC];
  const size_t n = blockIdx.x, row_elems = (size_t)p.S * p.C;
  const float* xb = x + n * row_elems;
  channel_moments(xb, 0, p.S, p, ch, sc);
  const int t = threadIdx.x;
  const bool wave = p.D > kSerialEntries;
  for (int g = wave ? t >> 6 : t; g < p.G; g += wave ? kThreads / 64 : kThreads) {
    float mean, rstd;
    group_moments(ch, 0, g, p, wave ? t & 63 : 0, wave ? 64 : 1, wave ? kByWave : kByThread, nullptr, mean, rstd);
    if (!wave || (t & 63) == 0) {
      gs[g] = mean; gs[kFusedMaxC + g] = rstd;
      if (mean_out) { mean_out[n * p.G + g] = mean; rstd_out[n * p.G + g] = rstd; }
    }
  }
  __syncthreads();
  apply_fwd(xb, y + n * row_elems, 0, p.S, p, gs, gs + kFusedMaxC, scale, shift);
}

__global__ __launch_bounds__(kThreads) void gn_bwd_fused_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ scale, float* __restrict__ dx,
                                                                float* __restrict__ part_rows, Geo p) {
  __shared__ Scratch sc;
  __shared__ float part[2 * kFusedMaxC];
  __shared__ float gs[2 * kFusedMaxC];
  const size_t n = blockIdx.x, row_elems = (size_t)p.S * p.C;
  const float* xb = x + n * row_elems;
  const float* dyb = dy + n * row_elems;
  const float* gm = mean + n * p.G;
  const float* gr = rstd + n * p.G;
  channel_grad_sums(dyb, xb, 0, p.S, p, gm, gr, part, sc);
  const int t = threadIdx.x;
  if (part_rows)
    for (int i = t; i < 2 * p.C; i += kThreads) part_rows[n * 2 * p.C + i] = part[i];
  const bool wave = p.D > kSerialEntries;
  for (int g = wave ? t >> 6 : t; g < p.G; g += wave ? kThreads / 64 : kThreads) {
    float ga, gb;
    group_grad_means(part, 0, g, p, scale, wave ? t & 63 : 0, wave ? 64 : 1, wave ? kByWave : kByThread, nullptr, ga, gb);
    if (!wave || (t & 63) == 0) { gs[g] = ga; gs[kFusedMaxC + g] = gb; }
  }
  __syncthreads();
  apply_bwd(dyb, xb, dx + n * row_elems, 0, p.S, p, gm, gr, gs, gs + kFusedMaxC, scale);
}

// ---- a batch row over K blocks ------------------------------------------------------------------------------------------------
// block n K + k: the chunk-channel moments of rows k rpc .. of batch row n -> rows[n K + k] = (mean[C], M2[C])
__global__ __launch_bounds__(kThreads) void gn_chunk_moments_kernel(const float* __restrict__ x, float* __restrict__ rows, Geo p) {
  __shared__ Scratch sc;
  const size_t n = blockIdx.x / p.K;
  const int k = (int)(blockIdx.x - n * p.K);
  channel_moments(x + n * (size_t)p.S * p.C, k * p.rpc, k * p.rpc + rows_of(p, k), p, rows + (size_t)blockIdx.x * 2 * p.C, sc);
}

// a thread, a wavefront or a block per (batch row, group), by the number of chunk-channels to merge: mean, rstd [N, G]
__global__ __launch_bounds__(kThreads) void gn_group_moments_kernel(const float* __restrict__ rows, float* __restrict__ mean,
                                                                    float* __restrict__ rstd, size_t n_groups, Geo p) {
  __shared__ float lds[kThreads / 64];
  const int mode = merge_mode(p.K * p.D);
  const size_t tid = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t ng = mode == kByThread ? tid : (mode == kByWave ? tid >> 6 : blockIdx.x);
  if (ng >= n_groups) return;                     // whole wavefronts leave together; kByBlock: the grid is n_groups
  const size_t n = ng / p.G;
  const int g = (int)(ng - n * p.G);
  const int span = mode == kByThread ? 1 : (mode == kByWave ? 64 : kThreads);
  float m, r;
  group_moments(rows + n * p.K * 2 * p.C, 2 * p.C, g, p, threadIdx.x & (span - 1), span, mode, lds, m, r);
  if ((threadIdx.x & (span - 1)) == 0) { mean[ng] = m; rstd[ng] = r; }
}

__global__ __launch_bounds__(kThreads) void gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ y,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd, Geo p) {
  const size_t n = blockIdx.x / p.K;
  const int k = (int)(blockIdx.x - n * p.K);
  const size_t base = n * (size_t)p.S * p.C;
  apply_fwd(x + base, y + base, k * p.rpc, k * p.rpc + rows_of(p, k), p, mean + n * p.G, rstd + n * p.G, scale, shift);
}

// block n K + k: rows[n K + k] = (sum dy [C], sum dy xhat [C]) over the chunk
__global__ __launch_bounds__(kThreads) void gn_chunk_grad_sums_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                      float* __restrict__ rows, Geo p) {
  __shared__ Scratch sc;
  const size_t n = blockIdx.x / p.K;
  const int k = (int)(blockIdx.x - n * p.K);
  const size_t base = n * (size_t)p.S * p.C;
  channel_grad_sums(dy + base, x + base, k * p.rpc, k * p.rpc + rows_of(p, k), p, mean + n * p.G, rstd + n * p.G,
                    rows + (size_t)blockIdx.x * 2 * p.C, sc);
}

// a thread, a wavefront or a block per (batch row, group): group_means [2, N, G] = (mean g'), (mean g' xhat)
__global__ __launch_bounds__(kThreads) void gn_group_grad_means_kernel(const float* __restrict__ rows, const float* __restrict__ scale,
                                                                       float* __restrict__ group_means, size_t n_groups, Geo p) {
  __shared__ float lds[kThreads / 64];
  const int mode = merge_mode(p.K * p.D);
  const size_t tid = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t ng = mode == kByThread ? tid : (mode == kByWave ? tid >> 6 : blockIdx.x);
  if (ng >= n_groups) return;
  const size_t n = ng / p.G;
  const int g = (int)(ng - n * p.G);
  const int span = mode == kByThread ? 1 : (mode == kByWave ? 64 : kThreads);
  float ga, gb;
  group_grad_means(rows + n * p.K * 2 * p.C, 2 * p.C, g, p, scale, threadIdx.x & (span - 1), span, mode, lds, ga, gb);
  if ((threadIdx.x & (span - 1)) == 0) { group_means[n_groups + ng] = gb; group_means[ng] = ga; }
}

__global__ __launch_bounds__(kThreads) void gn_apply_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ scale, const float* __restrict__ group_means,
                                                                float* __restrict__ dx, size_t n_groups, Geo p) {
  const size_t n = blockIdx.x / p.K;
  const int k = (int)(blockIdx.x - n * p.K);
  const size_t base = n * (size_t)p.S * p.C;
  apply_bwd(dy + base, x + base, dx + base, k * p.rpc, k * p.rpc + rows_of(p, k), p, mean + n * p.G, rstd + n * p.G,
            group_means + n * p.G, group_means + n_groups + n * p.G, scale);
}

// dshift[c] = sum over the partial rows of row[c], dscale[c] of row[C + c], ascending
__global__ __launch_bounds__(kThreads) void gn_param_reduce_kernel(const float* __restrict__ rows, size_t n_rows, int C,
                                                                   float* __restrict__ dscale, float* __restrict__ dshift) {
  const int i = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);
  if (i >= 2 * C) return;
  float s = 0.0f;
  for (size_t r = 0; r < n_rows; ++r) s += rows[r * 2 * C + i];
  if (i < C) dshift[i] = s; else dscale[i - C] = s;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static inline int check_shape(size_t n, size_t s, int c, int groups) {
  if (c < 1 || groups < 1 || s < 1 || c % groups != 0) return DDSP_ERR_BAD_SHAPE;
  const size_t limit = (size_t)1 << 31;
  if (s >= limit || n >= limit || s * (size_t)c >= limit || n * (s * (size_t)c) >= limit) return DDSP_ERR_UNSUPPORTED;
  return DDSP_OK;
}

static inline Geo make_geo(size_t s, int c, int groups, float eps) {
  Geo p;
  p.S = (int)s; p.C = c; p.G = groups; p.D = c / groups; p.eps = eps;
  if (c <= kThreads) { p.TW = c; p.R = kThreads / c; p.tiles = 1; }
  else { p.TW = kThreads; p.R = 1; p.tiles = (c + kThreads - 1) / kThreads; }
  p.rpc = kChunkElems / c < 1 ? 1 : kChunkElems / c;
  if (p.rpc > p.S) p.rpc = p.S;
  p.K = (p.S + p.rpc - 1) / p.rpc;
  return p;
}

static inline bool one_block(const Geo& p) { return p.K == 1 && p.C <= kFusedMaxC; }

// the split path's workspace: [N K][2 C] partial rows, then [2][N G] group values
static inline size_t split_bytes(size_t n, const Geo& p) {
  return (n * p.K * 2 * (size_t)p.C + 2 * n * (size_t)p.G) * sizeof(float);
}

static inline unsigned group_blocks(size_t n_groups, const Geo& p) {
  const int entries = p.K * p.D;
  const size_t per_block = entries <= kSerialEntries ? kThreads : (entries < kBlockEntries ? kThreads / 64 : 1);
  return (unsigned)((n_groups + per_block - 1) / per_block);
}

}  // namespace norm
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::norm;

extern "C" size_t ddsp_group_norm_workspace_bytes(size_t n, size_t s, int c, int groups) {
  if (check_shape(n, s, c, groups) != DDSP_OK || n == 0) return 0;
  const Geo p = make_geo(s, c, groups, 0.0f);
  return one_block(p) ? 0 : split_bytes(n, p);
}

extern "C" int ddsp_group_norm_f32(const float* x, const float* scale, const float* shift, float* y, float* mean, float* rstd,
                                   void* workspace, size_t workspace_bytes, size_t n, size_t s, int c, int groups, float eps,
                                   void* stream) {
  if (!x || !y || (scale == nullptr) != (shift == nullptr) || (mean == nullptr) != (rstd == nullptr)) return DDSP_ERR_NULL_POINTER;
  if (!(eps >= 0.0f)) return DDSP_ERR_BAD_SHAPE;
  const int rc = check_shape(n, s, c, groups);
  if (rc != DDSP_OK) return rc;
  if (n == 0) return DDSP_OK;
  const Geo p = make_geo(s, c, groups, eps);
  hipStream_t st = (hipStream_t)stream;
  if (one_block(p)) {
    hipLaunchKernelGGL(gn_fwd_fused_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, x, scale, shift, y, mean, rstd, p);
    return check_launch();
  }
  if (!workspace) return DDSP_ERR_NULL_POINTER;
  if (workspace_bytes < split_bytes(n, p)) return DDSP_ERR_WORKSPACE;
  float* rows = static_cast<float*>(workspace);
  float* group_values = rows + n * p.K * 2 * (size_t)p.C;
  const size_t n_groups = n * (size_t)p.G;
  float* m = mean ? mean : group_values;
  float* r = rstd ? rstd : group_values + n_groups;
  const dim3 grid((unsigned)(n * p.K));
  hipLaunchKernelGGL(gn_chunk_moments_kernel, grid, dim3(kThreads), 0, st, x, rows, p);
  hipLaunchKernelGGL(gn_group_moments_kernel, dim3(group_blocks(n_groups, p)), dim3(kThreads), 0, st, rows, m, r, n_groups, p);
  hipLaunchKernelGGL(gn_apply_kernel, grid, dim3(kThreads), 0, st, x, scale, shift, y, m, r, p);
  return check_launch();
}

extern "C" size_t ddsp_group_norm_backward_workspace_bytes(size_t n, size_t s, int c, int groups) {
  if (check_shape(n, s, c, groups) != DDSP_OK || n == 0) return 0;
  const Geo p = make_geo(s, c, groups, 0.0f);
  return one_block(p) ? n * 2 * (size_t)c * sizeof(float) : split_bytes(n, p);
}

extern "C" int ddsp_group_norm_backward_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* scale,
                                            float* dx, float* dscale, float* dshift, void* workspace, size_t workspace_bytes, size_t n,
                                            size_t s, int c, int groups, void* stream) {
  if (!dy || !x || !mean || !rstd || !dx || (dscale == nullptr) != (dshift == nullptr) || (dscale && !scale)) return DDSP_ERR_NULL_POINTER;
  const int rc = check_shape(n, s, c, groups);
  if (rc != DDSP_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    if (!dscale) return DDSP_OK;
    const bool ok = hipMemsetAsync(dscale, 0, (size_t)c * sizeof(float), st) == hipSuccess &&
                    hipMemsetAsync(dshift, 0, (size_t)c * sizeof(float), st) == hipSuccess;
    return ok ? DDSP_OK : DDSP_ERR_LAUNCH;
  }
  const Geo p = make_geo(s, c, groups, 0.0f);
  const bool fused = one_block(p);
  if (!workspace && (!fused || dscale)) return DDSP_ERR_NULL_POINTER;
  if ((!fused || dscale) && workspace_bytes < ddsp_group_norm_backward_workspace_bytes(n, s, c, groups)) return DDSP_ERR_WORKSPACE;
  float* rows = static_cast<float*>(workspace);
  const dim3 reduce_grid((unsigned)((2 * c + kThreads - 1) / kThreads));
  if (fused) {
    hipLaunchKernelGGL(gn_bwd_fused_kernel, dim3((unsigned)n), dim3(kThreads), 0, st, dy, x, mean, rstd, scale, dx,
                       dscale ? rows : (float*)nullptr, p);
    if (dscale) hipLaunchKernelGGL(gn_param_reduce_kernel, reduce_grid, dim3(kThreads), 0, st, rows, n, c, dscale, dshift);
    return check_launch();
  }
  const size_t n_groups = n * (size_t)p.G;
  float* group_means = rows + n * p.K * 2 * (size_t)p.C;
  const dim3 grid((unsigned)(n * p.K));
  hipLaunchKernelGGL(gn_chunk_grad_sums_kernel, grid, dim3(kThreads), 0, st, dy, x, mean, rstd, rows, p);
  hipLaunchKernelGGL(gn_group_grad_means_kernel, dim3(group_blocks(n_groups, p)), dim3(kThreads), 0, st, rows, scale, group_means,
                     n_groups, p);
  if (dscale) hipLaunchKernelGGL(gn_param_reduce_kernel, reduce_grid, dim3(kThreads), 0, st, rows, n * p.K, c, dscale, dshift);
  hipLaunchKernelGGL(gn_apply_bwd_kernel, grid, dim3(kThreads), 0, st, dy, x, mean, rstd, scale, group_means, dx, n_groups, p);
  return check_launch();
}
