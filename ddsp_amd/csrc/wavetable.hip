// Wavetable synthesis and the modulated delay for gfx950: core.linear_lookup, core.wavetable_synthesis,
// core.variable_length_delay (ddsp/core.py:1167-1313), synths.Wavetable (ddsp/synths.py:199-258) and
// effects.ModDelay (ddsp/effects.py:327-392), forward and backward.
//
// The reference resamples the tables to audio rate ([B, N, W]), builds two more tensors of that size for the
// lookup weights, multiplies and reduces; variable_length_delay frames the audio into [B, N, max_length].  What
// is computed per output sample is a two-point lerp in one or two tables, so nothing of that size exists here:
//
//   wt_fused_kernel      synths.Wavetable's case (tables on the same F frames as f0 and the amplitudes,
//                        N % F == 0): a block walks a run of frames with the tables of frame j and j + 1 in LDS
//                        (each frame's table is read from HBM once per run), applies exp_sigmoid while it
//                        stages, and evaluates window envelope, phase and the 2 x 2 blend per sample.
//   wt_sample_kernel     every other table layout (Fw != F, static, audio rate, N % Fw != 0): the four table
//                        values are gathered from L2 / HBM; with BWD it writes what the backward kernels need.
//   lookup_*, delay_*    linear_lookup with the caller's phase; the delay reads its two taps from the audio.
//
// Phase: cycles, not radians.  The frame-rate frequencies are summed per frame in closed form (the linear
// upsampling makes a frame's samples an arithmetic series), the sum over the frames before a block's first one is
// taken in fp64, and the position inside the frame is the quadratic in fp64 too (the vector ALUs run fp64 FMAs at
// the fp32 rate and a sample needs four of them).  The cumulative sum is EXCLUSIVE (tf.cumsum(exclusive=True)):
// phase(0) = 0.
//
// The gradients with respect to tables and audio are scatters in the reference's graph.  Here they are gathers
// with a fixed order of additions (no floating-point atomics): a block per (row, table frame) walks the samples
// that can touch the frame in time order and every table point is owned by one thread; a thread per audio sample
// walks the max_length + 1 outputs that can have read it.  Same bits on every run and for any sub-batch.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "profile.h"
#include "launch.h"

namespace ddsp {
namespace wavetable {

constexpr int kThreads = 256;
constexpr int kFramesPerBlock = 8;          // wt_fused_kernel: frames per block (tables read (8 + 1) / 8 times)
constexpr int kMaxLdsTable = 8192;          // points per table the LDS kernels take (2 x 32 KB staged forward)
constexpr float kLn10 = 2.302585092994046f;

#if defined(__clang__)
#define DDSP_WT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DDSP_WT_NO_CONTRACT
#endif
__device__ __forceinline__ float rn_mul(float a, float b) { DDSP_WT_NO_CONTRACT return a * b; }

// core.exp_sigmoid with the default constants (2 sigmoid(x)^ln 10 + 1e-7) and its derivative
__device__ __forceinline__ float exp_sigmoid(float x) {
  const float ax = fabsf(x);
  const float sp_tail = __logf(1.0f + __expf(-ax));
  const float softplus_neg = (x >= 0.0f) ? sp_tail : (ax + sp_tail);
  return 2.0f * __expf(-kLn10 * softplus_neg) + 1e-7f;
}
__device__ __forceinline__ float exp_sigmoid_grad(float x) {
  const float ax = fabsf(x);
  const float e = __expf(-ax);
  const float sp_tail = __logf(1.0f + e);
  const float softplus_neg = (x >= 0.0f) ? sp_tail : (ax + sp_tail);
  const float one_minus_sigmoid = (x >= 0.0f) ? e / (1.0f + e) : 1.0f / (1.0f + e);
  return 2.0f * kLn10 * __expf(-kLn10 * softplus_neg) * one_minus_sigmoid;
}
__device__ __forceinline__ float sigmoid(float x) {
  const float e = __expf(-fabsf(x));
  return (x >= 0.0f) ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

struct WtArgs {
  int F, Fw, W, N, hop;      // hop = N / F
  float sample_rate;
  unsigned flags;
};

// ---- phase -----------------------------------------------------------------------------------------------
// Sum over the samples of frame j of the linearly upsampled frequency (Hz samples): the frame's samples are
// f_j + d r / hop, r = 0 .. hop - 1, d = f_{j+1} - f_j (the last frame is held).
__device__ __forceinline__ double frame_cycles(const float* __restrict__ f0, int j, int F, int hop) {
  const double fa = (double)f0[j], fb = (double)f0[min(j + 1, F - 1)];
  return (double)hop * fa + (fb - fa) * (0.5 * (double)(hop - 1));
}

// Sum of frame_cycles over frames [0, j_end) by the whole block, in a fixed order (every thread must call it).
__device__ double block_prefix(const float* __restrict__ f0, int j_end, int F, int hop, double* s_red /*[kThreads]*/) {
  double local = 0.0;
  for (int j = threadIdx.x; j < j_end; j += kThreads) local += frame_cycles(f0, j, F, hop);
  s_red[threadIdx.x] = local;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
    __syncthreads();
  }
  const double total = s_red[0];
  __syncthreads();
  return total;
}

// Table position of the sample r samples into frame j, `before` Hz samples accumulated up to the frame's start.
__device__ __forceinline__ void phase_position(double before, float fj, float fj1, int r, int hop, double inv_sr, int W,
                                               int& i0, float& frac) {
  const double rr = (double)r;
  const double hz = before + rr * (double)fj + ((double)fj1 - (double)fj) * (rr * (rr - 1.0)) * (0.5 / (double)hop);
  const double cyc = hz * inv_sr;
  const double x = (cyc - floor(cyc)) * (double)W;      // tf's floormod: [0, 1) also for negative frequencies
  i0 = max(min((int)x, W - 1), 0);                       // (a NaN frequency must not index outside the table)
  frac = (float)(x - (double)i0);
}

__device__ __forceinline__ float window_weight(int r, int hop) {     // the rising half of Hann(2 hop), as resample's 'window'
  return 0.5f - 0.5f * cospif((float)r / (float)hop);
}

// =====================================================================================
// Fused forward: tables [B, F, W] on the frames of f0 and the amplitudes
// =====================================================================================
template <bool SCALE>
__global__ __launch_bounds__(kThreads) void wt_fused_kernel(const float* __restrict__ amps /*[B,F]*/,
                                                            const float* __restrict__ tables /*[B,F,W]*/,
                                                            const float* __restrict__ f0 /*[B,F]*/,
                                                            float* __restrict__ out /*[B,N]*/, WtArgs p) {
  extern __shared__ __attribute__((aligned(16))) float s_tab[];       // [2][W]
  __shared__ double s_red[kThreads];
  const int b = blockIdx.y, j_first = blockIdx.x * kFramesPerBlock;
  const int j_last = min(j_first + kFramesPerBlock, p.F);
  const float* __restrict__ fb = f0 + (size_t)b * p.F;
  const float* __restrict__ ab = amps + (size_t)b * p.F;
  const float* __restrict__ tb = tables + (size_t)b * p.F * p.W;
  float* __restrict__ ob = out + (size_t)b * p.N;
  const int W = p.W, hop = p.hop;
  const double inv_sr = 1.0 / (double)p.sample_rate;

  double before = block_prefix(fb, j_first, p.F, hop, s_red);
  auto stage = [&](int j, float* __restrict__ dst) {
    const float* __restrict__ src = tb + (size_t)j * W;
    if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(tb) & 15) == 0) {     // (the caller's tables may start on any 4-byte boundary)
      for (int i = threadIdx.x * 4; i < W; i += kThreads * 4) {
        float4 v = *reinterpret_cast<const float4*>(src + i);
        if (SCALE) { v.x = exp_sigmoid(v.x); v.y = exp_sigmoid(v.y); v.z = exp_sigmoid(v.z); v.w = exp_sigmoid(v.w); }
        *reinterpret_cast<float4*>(dst + i) = v;
      }
    } else {
      for (int i = threadIdx.x; i < W; i += kThreads) dst[i] = SCALE ? exp_sigmoid(src[i]) : src[i];
    }
  };
  stage(j_first, s_tab);
  for (int j = j_first; j < j_last; ++j) {
    const int k = j - j_first;
    const float* __restrict__ cur = s_tab + (size_t)(k & 1) * W;
    float* __restrict__ nxt_w = s_tab + (size_t)((k + 1) & 1) * W;
    const int jn = min(j + 1, p.F - 1);
    if (jn != j) stage(jn, nxt_w);
    __syncthreads();
    const float* __restrict__ nxt = (jn != j) ? nxt_w : cur;
    const float fj = fb[j], fj1 = fb[jn];
    float aj = ab[j], aj1 = ab[jn];
    if (SCALE) { aj = exp_sigmoid(aj); aj1 = exp_sigmoid(aj1); }
    for (int r = threadIdx.x; r < hop; r += kThreads) {
      int i0; float frac;
      phase_position(before, fj, fj1, r, hop, inv_sr, W, i0, frac);
      const int i1 = (i0 + 1 == W) ? 0 : i0 + 1;
      const float c0 = cur[i0], c1 = cur[i1], n0 = nxt[i0], n1 = nxt[i1];
      const float vc = c0 + frac * (c1 - c0), vn = n0 + frac * (n1 - n0);
      const float wf = (float)r / (float)hop;
      const float ww = window_weight(r, hop);
      const float a = aj * (1.0f - ww) + aj1 * ww;
      ob[(size_t)j * hop + r] = a * (vc + wf * (vn - vc));
    }
    before += frame_cycles(fb, j, p.F, hop);
    __syncthreads();                       // the table of frame j is overwritten by the next step's staging
  }
}

// =====================================================================================
// General forward / the per-sample half of the backward pass: any table layout
//   table(t) is the legacy-bilinear blend of frames floor(t Fw / N) and the next (held at the end), the position
//   taken exactly (integers); Fw == 1 is a static table, Fw == N one table per sample.
// =====================================================================================
struct WtBwdOut {
  float* ga;       // [B,N] grad_out * lookup value          (-> amplitudes, through the window's adjoint)
  float* cphi;     // [B,N] dL/d phase(t) / sample_rate      (-> f0, through the reverse scan)
  int* i0;         // [B,N] lower table point
  float* c0;       // [B,N] grad_out * a * (1 - frac)        (-> table point i0)
  float* c1;       // [B,N] grad_out * a * frac              (-> table point i0 + 1)
};

__device__ __forceinline__ void table_frames(int t, int Fw, int N, int& jw, int& hi, float& wf) {
  const long long num = (long long)t * Fw;
  jw = (int)(num / N);
  const int rem = (int)(num - (long long)jw * N);
  hi = min(jw + 1, Fw - 1);
  wf = (float)((double)rem / (double)N);
}

template <bool SCALE, bool BWD>
__global__ __launch_bounds__(kThreads) void wt_sample_kernel(const float* __restrict__ amps, const float* __restrict__ tables,
                                                             const float* __restrict__ f0, const float* __restrict__ gout,
                                                             float* __restrict__ out, WtBwdOut bw, WtArgs p) {
  __shared__ double s_red[kThreads];
  const int b = blockIdx.y;
  const int t_first = blockIdx.x * kThreads;
  const float* __restrict__ fb = f0 + (size_t)b * p.F;
  const float* __restrict__ ab = amps + (size_t)b * p.F;
  const float* __restrict__ tb = tables + (size_t)b * p.Fw * p.W;
  const int hop = p.hop, W = p.W;
  const int j_first = t_first / hop;
  double before = block_prefix(fb, j_first, p.F, hop, s_red);
  const int t = t_first + threadIdx.x;
  if (t >= p.N) return;
  const int j = t / hop, r = t - j * hop;
  for (int jj = j_first; jj < j; ++jj) before += frame_cycles(fb, jj, p.F, hop);
  const int jn = min(j + 1, p.F - 1);
  int i0; float frac;
  phase_position(before, fb[j], fb[jn], r, hop, 1.0 / (double)p.sample_rate, W, i0, frac);
  const int i1 = (i0 + 1 == W) ? 0 : i0 + 1;
  int jw, hi; float wf;
  table_frames(t, p.Fw, p.N, jw, hi, wf);
  const float* __restrict__ cur = tb + (size_t)jw * W;
  const float* __restrict__ nxt = tb + (size_t)hi * W;
  float c0 = cur[i0], c1 = cur[i1], n0 = nxt[i0], n1 = nxt[i1];
  if (SCALE) { c0 = exp_sigmoid(c0); c1 = exp_sigmoid(c1); n0 = exp_sigmoid(n0); n1 = exp_sigmoid(n1); }
  const float vc = c0 + frac * (c1 - c0), vn = n0 + frac * (n1 - n0);
  const float v = vc + wf * (vn - vc);
  float aj = ab[j], aj1 = ab[jn];
  if (SCALE) { aj = exp_sigmoid(aj); aj1 = exp_sigmoid(aj1); }
  const float ww = window_weight(r, hop);
  const float a = aj * (1.0f - ww) + aj1 * ww;
  const size_t o = (size_t)b * p.N + t;
  if (!BWD) {
    out[o] = a * v;
  } else {
    const float g = gout[o];
    const float sc = c1 - c0, sn = n1 - n0;
    const float slope = sc + wf * (sn - sc);                 // d value / d (table position)
    bw.ga[o] = g * v;
    bw.cphi[o] = g * a * slope * ((float)W / p.sample_rate);
    bw.i0[o] = i0;
    bw.c0[o] = g * a * (1.0f - frac);
    bw.c1[o] = g * a * frac;
  }
}

// =====================================================================================
// Lookup with a given position
// =====================================================================================
// x = phase * L split as floor + fraction without losing the product's low bits (L need not be a power of two):
// hi + lo is the exact product.  Points outside [0, L] do not exist (their relu weight belongs to no table entry).
__device__ __forceinline__ void split_position(float phase, int L, int& i0, float& frac) {
  const float fl_L = (float)L;
  const float hi = rn_mul(phase, fl_L);
  // (a NaN or infinite position has no table entry either, and its fraction is a NaN - hi - hi, 0 for every finite hi -: the
  // lerp of the two missing points is then a NaN and not a 0)
  if (!(hi > -2.0f)) { i0 = -3; frac = hi - hi; return; }
  if (hi > fl_L + 2.0f) { i0 = L + 2; frac = hi - hi; return; }
  const float lo = fmaf(phase, fl_L, -hi);
  const float fl = floorf(hi);
  i0 = (int)fl;
  frac = (hi - fl) + lo;
  if (frac < 0.0f) { i0 -= 1; frac += 1.0f; }
  else if (frac >= 1.0f) { i0 += 1; frac -= 1.0f; }
}

__device__ __forceinline__ float table_point(const float* __restrict__ tab, int pnt, int W) {
  return (pnt >= 0 && pnt <= W) ? tab[pnt == W ? 0 : pnt] : 0.0f;
}

struct LookupArgs { int N, Fw, W; };

template <bool BWD>
__global__ __launch_bounds__(kThreads) void lookup_kernel(const float* __restrict__ phase /*[B,N]*/,
                                                          const float* __restrict__ tables /*[B,Fw,W], Fw in {1, N}*/,
                                                          const float* __restrict__ gout, float* __restrict__ out,
                                                          float* __restrict__ gphase, int* __restrict__ ws_i0,
                                                          float* __restrict__ ws_c0, float* __restrict__ ws_c1, LookupArgs p) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= p.N) return;
  const size_t o = (size_t)b * p.N + t;
  const float* __restrict__ tab = tables + ((size_t)b * p.Fw + (p.Fw == 1 ? 0 : t)) * p.W;
  int i0; float frac;
  split_position(phase[o], p.W, i0, frac);
  const float t0 = table_point(tab, i0, p.W), t1 = table_point(tab, i0 + 1, p.W);
  if (!BWD) {
    out[o] = t0 + frac * (t1 - t0);
  } else {
    const float g = gout[o];
    gphase[o] = g * (float)p.W * (t1 - t0);
    ws_i0[o] = i0;
    ws_c0[o] = g * (1.0f - frac);
    ws_c1[o] = g * frac;
  }
}

// dL/d tables[b, j, :] for any table layout.  Block (j, b); the samples whose table blend can involve frame j are
// walked in time order, 256 at a time through LDS; table point i is only ever added to by thread i % 256.
template <bool SCALE>
__global__ __launch_bounds__(kThreads) void table_grad_kernel(const int* __restrict__ ws_i0, const float* __restrict__ ws_c0,
                                                              const float* __restrict__ ws_c1,
                                                              const float* __restrict__ raw_tables /*SCALE: [B,Fw,W]*/,
                                                              float* __restrict__ gtables /*[B,Fw,W]*/, LookupArgs p) {
  extern __shared__ __attribute__((aligned(16))) float s_acc[];       // [W]
  __shared__ int s_i0[kThreads];
  __shared__ float s_a[kThreads], s_b[kThreads];
  const int j = blockIdx.x, b = blockIdx.y, W = p.W;
  for (int i = threadIdx.x; i < W; i += kThreads) s_acc[i] = 0.0f;
  // frames floor(t Fw / N) == j - 1 or j:  t in [ceil((j - 1) N / Fw), ceil((j + 1) N / Fw))
  const long long lo_num = (long long)max(j - 1, 0) * p.N, hi_num = (long long)(j + 1) * p.N;
  const int t_lo = (int)((lo_num + p.Fw - 1) / p.Fw);
  const int t_hi = (int)min((hi_num + p.Fw - 1) / p.Fw, (long long)p.N);
  for (int base = t_lo; base < t_hi; base += kThreads) {
    const int t = base + threadIdx.x;
    __syncthreads();
    if (t < t_hi) {
      int jw, hi; float wf;
      table_frames(t, p.Fw, p.N, jw, hi, wf);
      const float wgt = (jw == j ? 1.0f - wf : 0.0f) + (hi == j ? wf : 0.0f);
      const size_t o = (size_t)b * p.N + t;
      s_i0[threadIdx.x] = ws_i0[o];
      s_a[threadIdx.x] = ws_c0[o] * wgt;
      s_b[threadIdx.x] = ws_c1[o] * wgt;
    }
    __syncthreads();
    const int n = min(kThreads, t_hi - base);
    for (int k = 0; k < n; ++k) {
      const int p0 = s_i0[k], p1 = p0 + 1;
      if (p0 >= 0 && p0 <= W) {
        const int idx = (p0 == W) ? 0 : p0;
        if ((idx & (kThreads - 1)) == (int)threadIdx.x) s_acc[idx] += s_a[k];
      }
      if (p1 >= 0 && p1 <= W) {
        const int idx = (p1 == W) ? 0 : p1;
        if ((idx & (kThreads - 1)) == (int)threadIdx.x) s_acc[idx] += s_b[k];
      }
    }
  }
  const size_t row = ((size_t)b * p.Fw + j) * W;
  for (int i = threadIdx.x; i < W; i += kThreads)       // thread i % 256 reads back what it alone wrote
    gtables[row + i] = SCALE ? s_acc[i] * exp_sigmoid_grad(raw_tables[row + i]) : s_acc[i];
}

// dL/d amplitudes[b, j]: the adjoint of the window upsampling on ga (frame j fades in over frame j - 1's samples
// and out over its own; the last frame is held), then exp_sigmoid's derivative.
template <bool SCALE>
__global__ __launch_bounds__(kThreads) void amp_grad_kernel(const float* __restrict__ ga /*[B,N]*/, const float* __restrict__ amps,
                                                            float* __restrict__ gamps /*[B,F]*/, WtArgs p) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.F) return;
  const float* __restrict__ gb = ga + (size_t)b * p.N;
  float acc = 0.0f;
  const int t_lo = max(j - 1, 0) * p.hop, t_hi = (j + 1) * p.hop;
  for (int t = t_lo; t < t_hi; ++t) {
    const int jj = t / p.hop, r = t - jj * p.hop;
    const float w = window_weight(r, p.hop);
    const float g = gb[t];
    if (jj == j) acc = fmaf(g, 1.0f - w, acc);
    if (min(jj + 1, p.F - 1) == j) acc = fmaf(g, w, acc);
  }
  const size_t o = (size_t)b * p.F + j;
  gamps[o] = SCALE ? acc * exp_sigmoid_grad(amps[o]) : acc;
}

// dL/d f0: phase(t) = sum_{s < t} f(s) / sr, so dL/d f(s) = S(s) = sum_{u > s} cphi[u]; then the adjoint of the
// linear upsampling.  Frame sums and the suffix over the frames in fp64.
__global__ __launch_bounds__(kThreads) void f0_frame_sums_kernel(const float* __restrict__ cphi /*[B,N]*/,
                                                                 double* __restrict__ sums /*[B,F]*/, WtArgs p) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.F) return;
  const float* __restrict__ cb = cphi + (size_t)b * p.N + (size_t)j * p.hop;
  double acc = 0.0;
  for (int r = 0; r < p.hop; ++r) acc += (double)cb[r];
  sums[(size_t)b * p.F + j] = acc;
}

// in place: sums[b, j] <- sum over the frames after j.  One block per row; a thread owns a run of frames.
__global__ __launch_bounds__(kThreads) void f0_suffix_kernel(double* __restrict__ sums /*[B,F]*/, int F) {
  __shared__ double s_run[kThreads];
  double* __restrict__ sb = sums + (size_t)blockIdx.x * F;
  const int per = (F + kThreads - 1) / kThreads;
  const int j_lo = min((int)threadIdx.x * per, F), j_hi = min(j_lo + per, F);
  double local = 0.0;
  for (int j = j_lo; j < j_hi; ++j) local += sb[j];
  s_run[threadIdx.x] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    double after = 0.0;
    for (int k = kThreads - 1; k >= 0; --k) { const double mine = s_run[k]; s_run[k] = after; after += mine; }
  }
  __syncthreads();
  double after = s_run[threadIdx.x];
  for (int j = j_hi - 1; j >= j_lo; --j) { const double mine = sb[j]; sb[j] = after; after += mine; }
}

__global__ __launch_bounds__(kThreads) void f0_grad_kernel(const float* __restrict__ cphi /*[B,N]*/,
                                                           const double* __restrict__ after /*[B,F]*/,
                                                           float* __restrict__ gf0 /*[B,F]*/, WtArgs p) {
  const int b = blockIdx.y;
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.F) return;
  const float* __restrict__ cb = cphi + (size_t)b * p.N;
  const double inv_hop = 1.0 / (double)p.hop;
  double acc = 0.0;
  for (int jj = max(j - 1, 0); jj <= j; ++jj) {
    const bool lower = (jj == j), upper = (min(jj + 1, p.F - 1) == j);
    double run = after[(size_t)b * p.F + jj];
    for (int r = p.hop - 1; r >= 0; --r) {
      const double wf = (double)r * inv_hop;
      if (lower) acc += run * (1.0 - wf);
      if (upper) acc += run * wf;
      run += (double)cb[(size_t)jj * p.hop + r];
    }
  }
  gf0[(size_t)b * p.F + j] = (float)acc;
}

// =====================================================================================
// variable_length_delay / ModDelay
// =====================================================================================
struct DelayArgs {
  int N, L;
  float phase_scale, phase_offset;     // ModDelay: phase * depth / max + center / max
  unsigned flags;
};

__device__ __forceinline__ float delay_tap(const float* __restrict__ audio, int n, int pnt, int L) {
  if (pnt < 0 || pnt > L) return 0.0f;
  if (pnt == L) return audio[n];                     // the appended wrap point reads the undelayed sample
  return (n - pnt >= 0) ? audio[n - pnt] : 0.0f;
}

template <bool BWD>
__global__ __launch_bounds__(kThreads) void delay_kernel(const float* __restrict__ phase, const float* __restrict__ audio,
                                                         const float* __restrict__ gain, const float* __restrict__ gout,
                                                         float* __restrict__ out, float* __restrict__ gphase,
                                                         float* __restrict__ ggain, int* __restrict__ ws_i0,
                                                         float* __restrict__ ws_c0, float* __restrict__ ws_c1, DelayArgs p) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= p.N) return;
  const size_t o = (size_t)b * p.N + n;
  const float* __restrict__ xb = audio + (size_t)b * p.N;
  const float ph_raw = phase[o];
  const float ph_in = (p.flags & DDSP_DELAY_PHASE_SIGMOID) ? sigmoid(ph_raw) : ph_raw;
  const float ph = fmaf(ph_in, p.phase_scale, p.phase_offset);
  const float g_raw = gain ? gain[o] : 1.0f;
  const float gn = (gain && (p.flags & DDSP_DELAY_GAIN_EXP_SIGMOID)) ? exp_sigmoid(g_raw) : g_raw;
  int i0; float frac;
  split_position(ph, p.L, i0, frac);
  const float t0 = delay_tap(xb, n, i0, p.L), t1 = delay_tap(xb, n, i0 + 1, p.L);
  const float wet = t0 + frac * (t1 - t0);
  if (!BWD) {
    out[o] = (p.flags & DDSP_DELAY_ADD_DRY) ? wet * gn + xb[n] : wet * gn;
  } else {
    const float g = gout[o];
    float dph = g * gn * (float)p.L * (t1 - t0) * p.phase_scale;
    if (p.flags & DDSP_DELAY_PHASE_SIGMOID) dph *= ph_in * (1.0f - ph_in);
    gphase[o] = dph;
    if (ggain) ggain[o] = (p.flags & DDSP_DELAY_GAIN_EXP_SIGMOID) ? g * wet * exp_sigmoid_grad(g_raw) : g * wet;
    ws_i0[o] = i0;
    ws_c0[o] = g * gn * (1.0f - frac);
    ws_c1[o] = g * gn * frac;
  }
}

// dL/d audio[b, m]: output n = m + d read this sample as point d (d < L) if its position fell in [d - 1, d + 1);
// output m read it as point L as well.  Walked in the order d = 0 .. L - 1, then the wrap point, then the dry path.
__global__ __launch_bounds__(kThreads) void delay_audio_grad_kernel(const int* __restrict__ ws_i0, const float* __restrict__ ws_c0,
                                                                    const float* __restrict__ ws_c1, const float* __restrict__ gout,
                                                                    float* __restrict__ gaudio, DelayArgs p) {
  const int b = blockIdx.y;
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= p.N) return;
  const size_t row = (size_t)b * p.N;
  float acc = 0.0f;
  const int d_end = min(p.L, p.N - m);
  for (int d = 0; d < d_end; ++d) {
    const int i0 = ws_i0[row + m + d];
    if (i0 == d) acc += ws_c0[row + m + d];
    if (i0 + 1 == d) acc += ws_c1[row + m + d];
  }
  const int i0 = ws_i0[row + m];
  if (i0 == p.L) acc += ws_c0[row + m];
  if (i0 + 1 == p.L) acc += ws_c1[row + m];
  if (p.flags & DDSP_DELAY_ADD_DRY) acc += gout[row + m];
  gaudio[row + m] = acc;
}

static inline size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }
static inline unsigned blocks_for(int n) { return (unsigned)((n + kThreads - 1) / kThreads); }

static int check_wt_shape(int B, int F, int Fw, int W, int N, float sample_rate) {
  if (B <= 0 || F <= 0 || Fw <= 0 || W <= 0 || N <= 0 || B > 65535 || !(sample_rate > 0.0f)) return DDSP_ERR_BAD_SHAPE;
  if (N % F != 0 || F + 1 >= N) return DDSP_ERR_BAD_SHAPE;         // the 'window' envelope of the amplitudes (core.py:677-693)
  return DDSP_OK;
}

// sample-rate scratch of the backward passes: i0, c0, c1 (+ ga, cphi and the fp64 frame sums for the synthesis)
static size_t sample_ws_bytes(int B, int N, int arrays) { return align_up((size_t)B * N * 4, 16) * arrays; }

}  // namespace wavetable
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::wavetable;

extern "C" int ddsp_wavetable_f32(const float* amplitudes, const float* wavetables, const float* f0_hz, float* audio, int B,
                                  int F, int Fw, int W, int N, float sample_rate, unsigned flags, void* stream) {
  if (!amplitudes || !wavetables || !f0_hz || !audio) return DDSP_ERR_NULL_POINTER;
  const int rc = check_wt_shape(B, F, Fw, W, N, sample_rate);
  if (rc != DDSP_OK) return rc;
  WtArgs p;
  p.F = F; p.Fw = Fw; p.W = W; p.N = N; p.hop = N / F; p.sample_rate = sample_rate; p.flags = flags;
  const hipStream_t st = (hipStream_t)stream;
  const bool scale = (flags & DDSP_WT_SCALE_EXP_SIGMOID) != 0;
  if (Fw == F && W <= kMaxLdsTable) {
    const dim3 grid((unsigned)((F + kFramesPerBlock - 1) / kFramesPerBlock), (unsigned)B);
    const size_t lds = (size_t)2 * W * sizeof(float);
    hipEvent_t ev0, ev1;
    profile_kernel_events(kWavetableFused, &ev0, &ev1);
    if (scale)
      hipExtLaunchKernelGGL((wt_fused_kernel<true>), grid, dim3(kThreads), lds, st, ev0, ev1, 0, amplitudes, wavetables, f0_hz,
                            audio, p);
    else
      hipExtLaunchKernelGGL((wt_fused_kernel<false>), grid, dim3(kThreads), lds, st, ev0, ev1, 0, amplitudes, wavetables, f0_hz,
                            audio, p);
    return check_launch();
  }
  const dim3 grid(blocks_for(N), (unsigned)B);
  const WtBwdOut none = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (scale)
    hipLaunchKernelGGL((wt_sample_kernel<true, false>), grid, dim3(kThreads), 0, st, amplitudes, wavetables, f0_hz,
                       (const float*)nullptr, audio, none, p);
  else
    hipLaunchKernelGGL((wt_sample_kernel<false, false>), grid, dim3(kThreads), 0, st, amplitudes, wavetables, f0_hz,
                       (const float*)nullptr, audio, none, p);
  return check_launch();
}

extern "C" size_t ddsp_wavetable_backward_workspace_bytes(int B, int F, int Fw, int W, int N) {
  (void)Fw; (void)W;
  if (B <= 0 || F <= 0 || N <= 0) return 0;
  return sample_ws_bytes(B, N, 5) + align_up((size_t)B * F * sizeof(double), 16);
}

extern "C" int ddsp_wavetable_backward_f32(const float* amplitudes, const float* wavetables, const float* f0_hz,
                                           const float* grad_audio, float* grad_amplitudes, float* grad_wavetables,
                                           float* grad_f0_hz, void* workspace, size_t workspace_bytes, int B, int F, int Fw,
                                           int W, int N, float sample_rate, unsigned flags, void* stream) {
  if (!amplitudes || !wavetables || !f0_hz || !grad_audio || !grad_amplitudes || !grad_wavetables || !grad_f0_hz || !workspace)
    return DDSP_ERR_NULL_POINTER;
  const int rc = check_wt_shape(B, F, Fw, W, N, sample_rate);
  if (rc != DDSP_OK) return rc;
  if (W > 2 * kMaxLdsTable) return DDSP_ERR_UNSUPPORTED;            // table_grad_kernel keeps one table in LDS
  if (workspace_bytes < ddsp_wavetable_backward_workspace_bytes(B, F, Fw, W, N) || ((uintptr_t)workspace & 15))
    return DDSP_ERR_WORKSPACE;
  WtArgs p;
  p.F = F; p.Fw = Fw; p.W = W; p.N = N; p.hop = N / F; p.sample_rate = sample_rate; p.flags = flags;
  const hipStream_t st = (hipStream_t)stream;
  const bool scale = (flags & DDSP_WT_SCALE_EXP_SIGMOID) != 0;
  const size_t stride = sample_ws_bytes(B, N, 1);
  char* ws = (char*)workspace;
  WtBwdOut bw;
  bw.ga = (float*)ws; bw.cphi = (float*)(ws + stride); bw.i0 = (int*)(ws + 2 * stride);
  bw.c0 = (float*)(ws + 3 * stride); bw.c1 = (float*)(ws + 4 * stride);
  double* sums = (double*)(ws + 5 * stride);
  const dim3 sgrid(blocks_for(N), (unsigned)B), fgrid(blocks_for(F), (unsigned)B);
  if (scale)
    hipLaunchKernelGGL((wt_sample_kernel<true, true>), sgrid, dim3(kThreads), 0, st, amplitudes, wavetables, f0_hz, grad_audio,
                       (float*)nullptr, bw, p);
  else
    hipLaunchKernelGGL((wt_sample_kernel<false, true>), sgrid, dim3(kThreads), 0, st, amplitudes, wavetables, f0_hz, grad_audio,
                       (float*)nullptr, bw, p);
  LookupArgs lp;
  lp.N = N; lp.Fw = Fw; lp.W = W;
  const dim3 tgrid((unsigned)Fw, (unsigned)B);
  const size_t lds = (size_t)W * sizeof(float);
  if (scale) {
    hipLaunchKernelGGL((table_grad_kernel<true>), tgrid, dim3(kThreads), lds, st, bw.i0, bw.c0, bw.c1, wavetables, grad_wavetables, lp);
    hipLaunchKernelGGL((amp_grad_kernel<true>), fgrid, dim3(kThreads), 0, st, bw.ga, amplitudes, grad_amplitudes, p);
  } else {
    hipLaunchKernelGGL((table_grad_kernel<false>), tgrid, dim3(kThreads), lds, st, bw.i0, bw.c0, bw.c1, (const float*)nullptr,
                       grad_wavetables, lp);
    hipLaunchKernelGGL((amp_grad_kernel<false>), fgrid, dim3(kThreads), 0, st, bw.ga, amplitudes, grad_amplitudes, p);
  }
  hipLaunchKernelGGL(f0_frame_sums_kernel, fgrid, dim3(kThreads), 0, st, bw.cphi, sums, p);
  hipLaunchKernelGGL(f0_suffix_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, sums, F);
  hipLaunchKernelGGL(f0_grad_kernel, fgrid, dim3(kThreads), 0, st, bw.cphi, sums, grad_f0_hz, p);
  return check_launch();
}

static int check_lookup_shape(int B, int N, int Fw, int W) {
  if (B <= 0 || N <= 0 || W <= 0 || B > 65535) return DDSP_ERR_BAD_SHAPE;
  if (Fw != 1 && Fw != N) return DDSP_ERR_BAD_SHAPE;
  return DDSP_OK;
}

extern "C" int ddsp_linear_lookup_f32(const float* phase, const float* wavetables, float* out, int B, int N, int Fw, int W,
                                      void* stream) {
  if (!phase || !wavetables || !out) return DDSP_ERR_NULL_POINTER;
  const int rc = check_lookup_shape(B, N, Fw, W);
  if (rc != DDSP_OK) return rc;
  LookupArgs p;
  p.N = N; p.Fw = Fw; p.W = W;
  hipLaunchKernelGGL((lookup_kernel<false>), dim3(blocks_for(N), (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, phase,
                     wavetables, (const float*)nullptr, out, (float*)nullptr, (int*)nullptr, (float*)nullptr, (float*)nullptr, p);
  return check_launch();
}

extern "C" size_t ddsp_linear_lookup_backward_workspace_bytes(int B, int N) {
  return (B <= 0 || N <= 0) ? 0 : sample_ws_bytes(B, N, 3);
}

extern "C" int ddsp_linear_lookup_backward_f32(const float* phase, const float* wavetables, const float* grad_out,
                                               float* grad_phase, float* grad_wavetables, void* workspace,
                                               size_t workspace_bytes, int B, int N, int Fw, int W, void* stream) {
  if (!phase || !wavetables || !grad_out || !grad_phase || !grad_wavetables || !workspace) return DDSP_ERR_NULL_POINTER;
  const int rc = check_lookup_shape(B, N, Fw, W);
  if (rc != DDSP_OK) return rc;
  if (W > 2 * kMaxLdsTable) return DDSP_ERR_UNSUPPORTED;
  if (workspace_bytes < ddsp_linear_lookup_backward_workspace_bytes(B, N) || ((uintptr_t)workspace & 15)) return DDSP_ERR_WORKSPACE;
  LookupArgs p;
  p.N = N; p.Fw = Fw; p.W = W;
  const size_t stride = sample_ws_bytes(B, N, 1);
  char* ws = (char*)workspace;
  int* i0 = (int*)ws;
  float* c0 = (float*)(ws + stride);
  float* c1 = (float*)(ws + 2 * stride);
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((lookup_kernel<true>), dim3(blocks_for(N), (unsigned)B), dim3(kThreads), 0, st, phase, wavetables, grad_out,
                     (float*)nullptr, grad_phase, i0, c0, c1, p);
  hipLaunchKernelGGL((table_grad_kernel<false>), dim3((unsigned)Fw, (unsigned)B), dim3(kThreads), (size_t)W * sizeof(float), st, i0,
                     c0, c1, (const float*)nullptr, grad_wavetables, p);
  return check_launch();
}

static int check_delay_shape(int B, int N, int L) {
  if (B <= 0 || N <= 0 || L <= 0 || B > 65535 || L > (1 << 24)) return DDSP_ERR_BAD_SHAPE;
  return DDSP_OK;
}

extern "C" int ddsp_variable_length_delay_f32(const float* phase, const float* audio, const float* gain, float* out, int B, int N,
                                              int max_length, float phase_scale, float phase_offset, unsigned flags,
                                              void* stream) {
  if (!phase || !audio || !out) return DDSP_ERR_NULL_POINTER;
  const int rc = check_delay_shape(B, N, max_length);
  if (rc != DDSP_OK) return rc;
  DelayArgs p;
  p.N = N; p.L = max_length; p.phase_scale = phase_scale; p.phase_offset = phase_offset; p.flags = flags;
  hipLaunchKernelGGL((delay_kernel<false>), dim3(blocks_for(N), (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, phase, audio,
                     gain, (const float*)nullptr, out, (float*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr,
                     (float*)nullptr, p);
  return check_launch();
}

extern "C" size_t ddsp_variable_length_delay_backward_workspace_bytes(int B, int N) {
  return (B <= 0 || N <= 0) ? 0 : sample_ws_bytes(B, N, 3);
}

extern "C" int ddsp_variable_length_delay_backward_f32(const float* phase, const float* audio, const float* gain,
                                                       const float* grad_out, float* grad_phase, float* grad_audio,
                                                       float* grad_gain, void* workspace, size_t workspace_bytes, int B, int N,
                                                       int max_length, float phase_scale, float phase_offset, unsigned flags,
                                                       void* stream) {
  if (!phase || !audio || !grad_out || !grad_phase || !grad_audio || !workspace) return DDSP_ERR_NULL_POINTER;
  if ((gain == nullptr) != (grad_gain == nullptr)) return DDSP_ERR_NULL_POINTER;
  const int rc = check_delay_shape(B, N, max_length);
  if (rc != DDSP_OK) return rc;
  if (workspace_bytes < ddsp_variable_length_delay_backward_workspace_bytes(B, N) || ((uintptr_t)workspace & 15))
    return DDSP_ERR_WORKSPACE;
  DelayArgs p;
  p.N = N; p.L = max_length; p.phase_scale = phase_scale; p.phase_offset = phase_offset; p.flags = flags;
  const size_t stride = sample_ws_bytes(B, N, 1);
  char* ws = (char*)workspace;
  int* i0 = (int*)ws;
  float* c0 = (float*)(ws + stride);
  float* c1 = (float*)(ws + 2 * stride);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks_for(N), (unsigned)B);
  hipLaunchKernelGGL((delay_kernel<true>), grid, dim3(kThreads), 0, st, phase, audio, gain, grad_out, (float*)nullptr, grad_phase,
                     grad_gain, i0, c0, c1, p);
  hipLaunchKernelGGL(delay_audio_grad_kernel, grid, dim3(kThreads), 0, st, i0, c0, c1, grad_out, grad_audio, p);
  return check_launch();
}
