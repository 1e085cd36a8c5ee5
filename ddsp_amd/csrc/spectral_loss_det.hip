// The reproducible gradient of losses.SpectralLoss (opt-in: SpectralLoss(deterministic=True), the ..._det_f32 entry points of
// include/ddsp_amd.h): the SLAB instances of the gradient kernels of csrc/spectral_loss.hip and the gather behind them - "a
// store pass plus a per-destination sum pass" in place of fp32 atomics.  The blocks are the templates of spectral_loss_blocks.h
// (which says why this is a translation unit of its own); sizes, workspaces and argument checks are in spectral_loss.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "fft_radix8.h"
#include "spectral_loss_blocks.h"

namespace ddsp {

// The slab instances of stft_l1_bwd_kernel and stft_cot_bwd_kernel<S> (SLAB: stft_l1_bwd_block).  slab_first.at[z]: the first
// float of scale z's slabs, z in the GRID's order (SlMulti: descending size).  Registers / LDS as compiled for gfx950 (.vgpr_count,
// .sgpr_count, group segment; no instance spills):
//   stft_l1_bwd_slab_kernel          45 / 62 / 36 992 B   (the atomic instance: 44 / 60 / 36 992 - both inside the 64 registers of
//                                                          __launch_bounds__(512, 8))
//   stft_cot_bwd_slab_kernel<S>      32 - 45 / 30 - 33 / 36 864 B for S = 16 .. 4096
//   stft_l1_big_bwd_slab_kernel      109 / 58 / 36 992 B  (the atomic instance: the same)
//   stft_tq_cot_bwd_kernel<S, true>  36 - 49 / 42 - 46 / 36 864 B for S = 64 .. 8192
//   sl_grad_gather_kernel<V, ACCUM>  14 - 26 / 31 - 37 / no LDS
__global__ __launch_bounds__(kSlThreads, 8) void stft_l1_bwd_slab_kernel(const float* __restrict__ target, const float* __restrict__ audio,
                                                                      const float* __restrict__ grad_loss,
                                                                      float* __restrict__ slab, int N, SlMulti m,
                                                                      float safe_eps, double* __restrict__ partial,
                                                                      SlSlabFirst slab_first) {
  __shared__ __attribute__((aligned(16))) float2 s[kSlStore];
  __shared__ double red[2][kSlThreads / 64];
  int z, b, bx;
  if (!sl_where(m, (int)blockIdx.x, z, b, bx)) return;
  const int nbx = m.nbx[z];
  double* dst = partial ? partial + 2 * (size_t)m.offset[z] : nullptr;
  float* mine = slab + slab_first.at[z];
#define DDSP_SLS_BLOCK(SZ) case SZ: stft_l1_bwd_block<SZ, false, true>(s, red, target, audio, grad_loss, mine, N, m.frames[z], \
                                                                       safe_eps, m.mag_scale[z], m.log_scale[z], dst, nullptr, bx, b, nbx, \
                                                                       m.frame[z], m.hop_div[z]); break
  switch (m.size[z]) {
    DDSP_SLS_BLOCK(16); DDSP_SLS_BLOCK(32); DDSP_SLS_BLOCK(64); DDSP_SLS_BLOCK(128); DDSP_SLS_BLOCK(256);
    DDSP_SLS_BLOCK(512); DDSP_SLS_BLOCK(1024); DDSP_SLS_BLOCK(2048); DDSP_SLS_BLOCK(4096);
    default: break;
  }
#undef DDSP_SLS_BLOCK
}
template <int S>
__global__ __launch_bounds__(kSlThreads) void stft_cot_bwd_slab_kernel(const float* __restrict__ audio, float* __restrict__ slab,
                                                                       int N, int n_frames, const float* __restrict__ cot) {
  __shared__ __attribute__((aligned(16))) float2 s[kSlStore];
  stft_l1_bwd_block<S, true, true>(s, nullptr, audio, audio, nullptr, slab, N, n_frames, 1e-5f, 0.0f, 0.0f, nullptr, cot,
                                   (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x);
}

// the slab instance of stft_l1_big_bwd_kernel
__global__ __launch_bounds__(kSlThreads) void stft_l1_big_bwd_slab_kernel(const float* __restrict__ target, const float* __restrict__ audio,
                                                                          const float* __restrict__ grad_loss, float* __restrict__ slab,
                                                                          double* __restrict__ partial, int N, int n_frames, int F,
                                                                          float safe_eps, float mag_scale, float log_scale) {
  __shared__ __attribute__((aligned(16))) float2 s[kSlStore];
  __shared__ double red[2][kSlThreads / 64];
  stft_l1_big_block<true, true>(s, red, target, audio, grad_loss, slab, N, safe_eps, mag_scale, log_scale, partial, (int)blockIdx.x,
                                (int)blockIdx.y, n_frames, F, F / 4);
}

// ---- the reproducible gradient: a store pass plus a per-destination sum pass --------------------------------------------------
// The slab instances above store every block's stretch of partial sums to a slab of its own; this kernel adds, for each output
// sample, the few slabs that cover it - in a fixed order, in fp32, with no atomics and no LDS.  Two ordinary stream-ordered
// launches: nothing waits on another block, so the bits cannot depend on scheduling.
// THE ORDER (the contract; include/ddsp_amd.h and DESIGN.md section 8 state the same): for sample n of row b, g = 0 (ACCUM:
// g = grad_audio[b][n]); for each scale z in the order the caller lists them, t = 0, then t += slab value for the covering
// blocks in ASCENDING block index, then g += t; grad_audio[b][n] = g, written once.  Block bx of a scale covers the samples
// [bx step - pad, bx step - pad + stretch) and holds sample n at index n + pad - bx step of its slab.
// A thread owns V consecutive samples of one row.  V = 4 wherever step, stretch and pad are multiples of four (every scale of
// the fused path): the four samples then have the same covering blocks and each slab is read as one aligned 16-byte load;
// neighbouring lanes read neighbouring quads.  Slab floats whose sample lies outside the row are loaded with their quad and
// dropped, never added.
template <int V, bool ACCUM>
__global__ __launch_bounds__(kSlGatherThreads) void sl_grad_gather_kernel(const float* __restrict__ slab, float* __restrict__ grad_audio,
                                                                          int N, SlGather p) {
  static_assert(V == 1 || V == 4, "one sample or an aligned quad per thread");
  const int b = blockIdx.y;
  const long n0 = (long)V * ((long)blockIdx.x * kSlGatherThreads + threadIdx.x);
  if (n0 >= N) return;
  float* __restrict__ out = grad_audio + (size_t)b * N + n0;
  const bool whole = V == 1 || ((N & 3) == 0 && (reinterpret_cast<uintptr_t>(grad_audio) & 15) == 0);     // (else rows are not 16-byte aligned)
  float g[V];
#pragma unroll
  for (int v = 0; v < V; ++v) g[v] = 0.0f;
  if constexpr (ACCUM) {
    bool done = false;
    if constexpr (V == 4) {
      if (whole) { const float4 o = *reinterpret_cast<const float4*>(out); g[0] = o.x; g[1] = o.y; g[2] = o.z; g[3] = o.w; done = true; }
    }
    if (!done) {
#pragma unroll
      for (int v = 0; v < V; ++v) if (n0 + v < N) g[v] = out[v];
    }
  }
  for (int z = 0; z < p.n; ++z) {
    const int step = p.step[z], stretch = p.stretch[z], nbx = p.nbx[z];
    uint32_t r_;
    const int hi = (int)fastdiv((uint32_t)(n0 + p.pad[z]), p.step_div[z], r_), r = (int)r_;     // the last block that starts at or before n
    if (r >= stretch) continue;                                // (frames that leave gaps: nobody covers the sample)
    uint32_t unused;
    // block hi - k holds the sample at index r + k step: k from the block furthest back (ascending block index) to the nearest
    const int k_hi = min(hi, (int)fastdiv((uint32_t)(stretch - 1 - r), p.step_div[z], unused));
    const int k_lo = max(0, hi - (nbx - 1));
    const float* __restrict__ src = slab + p.first[z] + (long long)b * nbx * stretch;
    float t[V];
#pragma unroll
    for (int v = 0; v < V; ++v) t[v] = 0.0f;
    for (int k = k_hi; k >= k_lo; --k) {
      const float* __restrict__ at = src + (long long)(hi - k) * stretch + (r + k * step);
      if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(at);
        t[0] += q.x; t[1] += q.y; t[2] += q.z; t[3] += q.w;
      } else {
        t[0] += at[0];
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) g[v] += t[v];
  }
  if constexpr (V == 4) {
    if (whole) { *reinterpret_cast<float4*>(out) = make_float4(g[0], g[1], g[2], g[3]); return; }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) if (n0 + v < N) out[v] = g[v];
}

void sl_launch_gather(const float* slab, float* grad_audio, int B, int N, const SlGather& p, bool accum, hipStream_t st) {
  bool quads = true;
  for (int z = 0; z < p.n; ++z) quads = quads && !((p.step[z] | p.stretch[z] | p.pad[z]) & 3) && !(p.first[z] & 3);
  const int per = quads ? 4 : 1;
  const long long threads = ((long long)N + per - 1) / per;
  const dim3 grid((unsigned)((threads + kSlGatherThreads - 1) / kSlGatherThreads), (unsigned)B);
  if (quads) {
    if (accum) hipLaunchKernelGGL((sl_grad_gather_kernel<4, true>), grid, dim3(kSlGatherThreads), 0, st, slab, grad_audio, N, p);
    else hipLaunchKernelGGL((sl_grad_gather_kernel<4, false>), grid, dim3(kSlGatherThreads), 0, st, slab, grad_audio, N, p);
  } else {
    if (accum) hipLaunchKernelGGL((sl_grad_gather_kernel<1, true>), grid, dim3(kSlGatherThreads), 0, st, slab, grad_audio, N, p);
    else hipLaunchKernelGGL((sl_grad_gather_kernel<1, false>), grid, dim3(kSlGatherThreads), 0, st, slab, grad_audio, N, p);
  }
}


void sl_launch_l1_bwd_slab(unsigned grid, hipStream_t st, const float* target, const float* audio, const float* grad_loss,
                            float* slab, int N, const SlMulti& m, float safe_eps, double* partial, const SlSlabFirst& first) {
  hipLaunchKernelGGL(stft_l1_bwd_slab_kernel, dim3(grid), dim3(kSlThreads), 0, st, target, audio, grad_loss, slab, N, m, safe_eps,
                     partial, first);
}

void sl_launch_l1_big_bwd_slab(dim3 grid, hipStream_t st, const float* target, const float* audio, const float* grad_loss, float* slab,
                               double* partial, int N, int n_frames, int F, float safe_eps, float mag_scale, float log_scale) {
  hipLaunchKernelGGL(stft_l1_big_bwd_slab_kernel, grid, dim3(kSlThreads), 0, st, target, audio, grad_loss, slab, partial, N, n_frames,
                     F, safe_eps, mag_scale, log_scale);
}

bool sl_launch_cot_bwd_slab(int S, dim3 grid, hipStream_t st, const float* audio, float* slab, int N, int n_frames, const float* cot) {
#define DDSP_SMBD_CASE(SZ) case SZ: hipLaunchKernelGGL((stft_cot_bwd_slab_kernel<SZ>), grid, dim3(kSlThreads), 0, st, \
                                                       audio, slab, N, n_frames, cot); return true
  switch (S) {
    DDSP_SMBD_CASE(16); DDSP_SMBD_CASE(32); DDSP_SMBD_CASE(64); DDSP_SMBD_CASE(128); DDSP_SMBD_CASE(256);
    DDSP_SMBD_CASE(512); DDSP_SMBD_CASE(1024); DDSP_SMBD_CASE(2048); DDSP_SMBD_CASE(4096);
    default: return false;
  }
#undef DDSP_SMBD_CASE
}

bool sl_launch_tq_cot_bwd_slab(int S, dim3 grid, hipStream_t st, const float* audio, float* slab, int N, int n_frames,
                               const float* cot, SlFrameGeom fg) {
#define DDSP_SFBD_CASE(SZ) case SZ: hipLaunchKernelGGL((stft_tq_cot_bwd_kernel<SZ, true>), grid, dim3(kSlThreads), 0, st, audio, \
                                                       slab, N, n_frames, cot, fg); return true
  switch (S) {
    DDSP_SFBD_CASE(64); DDSP_SFBD_CASE(128); DDSP_SFBD_CASE(256); DDSP_SFBD_CASE(512); DDSP_SFBD_CASE(1024);
    DDSP_SFBD_CASE(2048); DDSP_SFBD_CASE(4096); DDSP_SFBD_CASE(8192);
    default: return false;
  }
#undef DDSP_SFBD_CASE
}

}  // namespace ddsp
