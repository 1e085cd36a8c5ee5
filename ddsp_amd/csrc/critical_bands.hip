// core.frequencies_critical_bands (ddsp/core.py:510-569), forward and backward in the network outputs:
//   out[r, k] = soft_limit(f_center[k] + bandwidth_scale * bw[k] * sum_d tanh(x[r, k, d]) * depth_modifier[d], hz_min, hz_max)
// x is [rows, K * depth] (a sinusoid's `depth` values side by side), out [rows, K]; f_center, bw [K] and depth_modifier
// [depth] are tables the host layer makes once per argument tuple.
//
// Layout.  x is one flat run of rows * K sinusoids of `depth` floats.  A block of 256 threads takes a TILE of consecutive
// sinusoids whose floats are one contiguous stretch of memory:
//   1. consecutive threads load consecutive floats of the stretch (every load instruction of a wavefront covers 256
//      contiguous bytes, whatever `depth` is), take the tanh and put it into LDS, sinusoid j's values from float
//      j * (chunk | 1) on: the odd stride keeps step 2 off a single bank;
//   2. thread j adds sinusoid j's values times depth_modifier in ascending d - one thread, one fixed order, nothing that
//      depends on where the row sits in the batch - and finishes the sinusoid; the K results of a row leave coalesced.
// The tile is the choice over sub-groups of a wavefront because it works for ANY depth (65 as well as 64, 3, 1) with one
// code path; a sub-group reduction needs a power of two or idle lanes.  A depth beyond 2048 goes through the same tile
// in chunks of 2048, the running sums staying in the threads' registers.
// The backward pass finds f the same way (so nothing but x is saved), keeps per sinusoid
//   coef = g_out * (sigmoid(f) - sigmoid(f - (hz_max - hz_min))) * bandwidth_scale * bw[k]
// in LDS and writes g_x[j, d] = coef_j * depth_modifier[d] * (1 - tanh^2) with the same coalesced indexing, the tanh read
// back from the tile (one chunk) or recomputed (several).
// tanh(x) = 1 - 2 / (e^2x + 1) on v_exp_f32 and v_rcp_f32: exact limits at both ends, an ABSOLUTE error of about 1.5e-7,
// which is what a sum that is then scaled by a bandwidth needs.  No atomics; the same bits for a row alone and in a batch.
// Bounds (DDSP_ERR_UNSUPPORTED beyond): rows * K below 2^31.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "common.h"
#include "launch.h"

namespace ddsp {
namespace critical_bands {

constexpr int kThreads = 256;
constexpr int kTileFloats = 4096;            // 16 KB: eight blocks (all 2048 threads) fit a CU
constexpr int kMaxChunk = 2048;              // depth values of a sinusoid in the tile at once
constexpr unsigned kMaxBlocks = 16384;
constexpr int kUnroll = 8;                   // loads a thread has in flight: 64 KB per CU, what 8 TB/s needs at ~2 us of latency

struct CbArgs {
  uint32_t n_sin;            // rows * K
  int depth, chunk, stride;  // chunk = min(depth, kMaxChunk); stride = chunk | 1
  int per_tile;              // sinusoids per tile: min(256, kTileFloats / stride)
  uint32_t n_tiles;
  FastDiv div_chunk, div_k;
  float scale, lo, width;    // bandwidth_scale, hz_min, hz_max - hz_min
};

__device__ __forceinline__ float fast_tanh(float x) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f);
}
__device__ __forceinline__ float softplus(float z) { return fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float sigmoid(float z) {
  const float e = expf(-fabsf(z)), s = 1.0f / (1.0f + e);
  return z >= 0.0f ? s : e * s;
}

template <bool BWD>
__global__ __launch_bounds__(kThreads) void critical_bands_kernel(const float* __restrict__ x, const float* __restrict__ g_out,
                                                                  float* __restrict__ out, const float* __restrict__ f_center,
                                                                  const float* __restrict__ bw, const float* __restrict__ dmod, CbArgs p) {
  __shared__ float tile[kTileFloats];
  __shared__ float coef[kThreads];
  const int tid = threadIdx.x;
  const bool one_chunk = p.chunk == p.depth;
  for (uint32_t t = blockIdx.x; t < p.n_tiles; t += gridDim.x) {
    const uint32_t s0 = t * (uint32_t)p.per_tile;
    const int ns = (int)min((uint32_t)p.per_tile, p.n_sin - s0);
    const float* __restrict__ xs = x + (size_t)s0 * (size_t)p.depth;
    const int span = ns * p.chunk;                                 // <= kTileFloats
    float acc = 0.0f;
    for (int c0 = 0; c0 < p.depth; c0 += p.chunk) {
      const int dc = min(p.chunk, p.depth - c0);
      // 1. the stretch -> tanh -> LDS
      for (int i0 = tid; i0 < span; i0 += kThreads * kUnroll) {
        float v[kUnroll];
        int at[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int i = i0 + u * kThreads;
          uint32_t d;
          const uint32_t j = fastdiv((uint32_t)i, p.div_chunk, d);
          const bool live = i < span && (int)d < dc;
          at[u] = live ? (int)j * p.stride + (int)d : -1;
          v[u] = live ? xs[(size_t)j * (size_t)p.depth + (size_t)(c0 + (int)d)] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
          if (at[u] >= 0) tile[at[u]] = fast_tanh(v[u]);
      }
      __syncthreads();
      // 2. one thread per sinusoid, ascending d
      if (tid < ns) {
        const float* __restrict__ mine = tile + tid * p.stride;
        for (int d = 0; d < dc; ++d) acc = fmaf(mine[d], dmod[c0 + d], acc);
      }
      if (!one_chunk) __syncthreads();                             // the tile is written again
    }
    float c = 0.0f;
    if (tid < ns) {
      uint32_t k;
      fastdiv(s0 + (uint32_t)tid, p.div_k, k);
      const float band = p.scale * bw[k];
      const float f = f_center[k] + band * acc;
      if (!BWD) {
        out[s0 + (uint32_t)tid] = (softplus(f) + p.lo) - softplus(f - p.width);      // core.soft_limit
      } else {
        c = g_out[s0 + (uint32_t)tid] * (sigmoid(f) - sigmoid(f - p.width)) * band;
      }
    }
    if (BWD) {
      coef[tid] = c;
      __syncthreads();
      float* __restrict__ gs = out + (size_t)s0 * (size_t)p.depth;
      for (int c0 = 0; c0 < p.depth; c0 += p.chunk) {
        const int dc = min(p.chunk, p.depth - c0);
        for (int i0 = tid; i0 < span; i0 += kThreads * kUnroll) {
          float th[kUnroll];
          size_t at[kUnroll];
          int jd[kUnroll][2];
#pragma unroll
          for (int u = 0; u < kUnroll; ++u) {
            const int i = i0 + u * kThreads;
            uint32_t d;
            const uint32_t j = fastdiv((uint32_t)i, p.div_chunk, d);
            const bool live = i < span && (int)d < dc;
            jd[u][0] = live ? (int)j : -1;
            jd[u][1] = c0 + (int)d;
            at[u] = (size_t)j * (size_t)p.depth + (size_t)(c0 + (int)d);
            th[u] = !live ? 0.0f : (one_chunk ? tile[(int)j * p.stride + (int)d] : fast_tanh(xs[at[u]]));
          }
#pragma unroll
          for (int u = 0; u < kUnroll; ++u)
            if (jd[u][0] >= 0) gs[at[u]] = coef[jd[u][0]] * dmod[jd[u][1]] * fmaf(-th[u], th[u], 1.0f);
        }
      }
    }
    __syncthreads();                                               // the next tile overwrites the LDS
  }
}

static bool plan(size_t rows, int K, int depth, float bandwidth_scale, float hz_min, float hz_max, CbArgs& p) {
  const size_t n_sin = rows * (size_t)K;
  if (n_sin > (size_t)0x7FFFFFFF) return false;
  p.n_sin = (uint32_t)n_sin;
  p.depth = depth;
  p.chunk = depth < kMaxChunk ? depth : kMaxChunk;
  p.stride = p.chunk | 1;
  p.per_tile = kTileFloats / p.stride;
  if (p.per_tile > kThreads) p.per_tile = kThreads;
  p.n_tiles = (uint32_t)((n_sin + (size_t)p.per_tile - 1) / (size_t)p.per_tile);
  p.div_chunk = make_fastdiv((uint32_t)p.chunk);
  p.div_k = make_fastdiv((uint32_t)K);
  p.scale = bandwidth_scale;
  p.lo = hz_min;
  p.width = (float)((double)hz_max - (double)hz_min);
  return true;
}

template <bool BWD>
static int run(const float* x, const float* g_out, float* out, const float* f_center, const float* bw, const float* dmod, size_t rows,
               int K, int depth, float bandwidth_scale, float hz_min, float hz_max, void* stream) {
  if (!x || !out || !f_center || !bw || !dmod || (BWD && !g_out)) return DDSP_ERR_NULL_POINTER;
  if (K < 1 || depth < 1) return DDSP_ERR_BAD_SHAPE;
  CbArgs p;
  if (!plan(rows, K, depth, bandwidth_scale, hz_min, hz_max, p)) return DDSP_ERR_UNSUPPORTED;
  if (rows == 0) return DDSP_OK;
  const unsigned grid = p.n_tiles < kMaxBlocks ? p.n_tiles : kMaxBlocks;
  hipLaunchKernelGGL(critical_bands_kernel<BWD>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, x, g_out, out, f_center, bw, dmod, p);
  return check_launch();
}

}  // namespace critical_bands
}  // namespace ddsp

using namespace ddsp;

extern "C" int ddsp_critical_bands_f32(const float* freqs, float* out, size_t rows, int K, int depth, const float* f_center,
                                       const float* bandwidths, const float* depth_modifier, float bandwidth_scale, float hz_min,
                                       float hz_max, void* stream) {
  return critical_bands::run<false>(freqs, nullptr, out, f_center, bandwidths, depth_modifier, rows, K, depth, bandwidth_scale, hz_min,
                                    hz_max, stream);
}

extern "C" int ddsp_critical_bands_backward_f32(const float* freqs, const float* grad_out, float* grad_freqs, size_t rows, int K,
                                                int depth, const float* f_center, const float* bandwidths,
                                                const float* depth_modifier, float bandwidth_scale, float hz_min, float hz_max,
                                                void* stream) {
  return critical_bands::run<true>(freqs, grad_out, grad_freqs, f_center, bandwidths, depth_modifier, rows, K, depth, bandwidth_scale,
                                   hz_min, hz_max, stream);
}
