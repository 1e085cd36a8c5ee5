// The blocks of the STFT kernels of csrc/spectral_loss.hip - the transforms of a block's frames in LDS, the loss and gradient
// arithmetic on them, the overlap-add epilogues - as templates two translation units instantiate: spectral_loss.hip (every
// forward kernel, and the gradient kernels that overlap-add with fp32 atomics) and spectral_loss_det.hip (the SLAB instances
// of the gradient kernels and the gather: the reproducible gradient).  Two units because the compiler's choices for a kernel
// depend on which other kernels it is compiled beside: with the slab instances in the same unit stft_l1_bwd_kernel came out with
// 42 registers and another instruction stream, alone it keeps the 44 and the stream it has been measured with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "fft_radix8.h"

namespace ddsp {

constexpr int kSlPoints = 4096;        // complex points per block (32 KB of LDS)
constexpr int kSlThreads = 512;
// LDS layout: 2 float2 of padding after every 16 (36 KB per block: four blocks still fit a CU) - a
// 16-element chunk then starts 36 dwords after the previous one, so the small-stride stages of the transforms (4 lanes per chunk, chunks 128 B apart)
// no longer land 8 or 16 lanes on the same banks; every index into the array goes through SP().
constexpr int kSlStore = kSlPoints + kSlPoints / 8;
__device__ __forceinline__ int SP(int i) { return i + ((i >> 4) << 1); }
      // 16 wavefronts per block: LDS and VALU phases of different wavefronts overlap (tools/microbench5)

// ---- the H-point transforms of all frames of a block, in place in LDS -----------------------------
// H = 2^L.  Forward = decimation in frequency in mixed radix: radix-8 stages first, then one or two radix-4 stages
// (3 n8 + 2 n4 = L): 17 passes over the LDS for the six sizes of the loss where radix-4 (+ a radix-2 stage for odd L)
// took 24.  A radix-8 stage is one butterfly per thread for the 4096 points of a block; in a radix-4 stage thread t
// takes butterflies 2 t and 2 t + 1 - so a frame belongs to the same threads in EVERY stage (frame g: threads
// g H/8 .. (g+1) H/8 - 1), and when that range lies inside one wavefront (H <= 512) a wavefront-level wait replaces the
// block barrier between stages.  Bin k ends up at sl_pos(k) (digit reversal in the stages' radices).
// The inverse is the algebraic inverse of those stages in reverse order, unscaled (H times the true inverse).
template <int H>
struct SlPlan {
  static constexpr int L = __builtin_ctz(H);
  static constexpr int N4 = (L % 3 == 0) ? 0 : ((L % 3 == 2) ? 1 : 2);       // L >= 3, or L = 2 (one radix-4 stage)
  static constexpr int N8 = (L - 2 * N4) / 3;
  static constexpr int M = 1 << (2 * N4);                  // the radix-4 part: what the radix-8 stages leave of a frame
  static constexpr bool kWaveLocal = (H / 8 >= 1) && (H / 8 <= 64);
  static_assert(3 * N8 + 2 * N4 == L, "stage plan");
};

template <int H>
__device__ __forceinline__ void sl_stage_sync() {
  if (SlPlan<H>::kWaveLocal) {
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

template <int H>
__device__ __forceinline__ int sl_pos(int k) {             // where bin k sits after sl_forward
  int p = 0, kk = k, m = H;
#pragma unroll
  for (int st = 0; st < SlPlan<H>::N8; ++st) { p += (kk & 7) * (m / 8); kk >>= 3; m >>= 3; }
#pragma unroll
  for (int st = 0; st < SlPlan<H>::N4; ++st) { p += (kk & 3) * (m / 4); kk >>= 2; m >>= 2; }
  return p;
}

__device__ __forceinline__ float2 sl_cmul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 sl_cmulc(float2 a, float2 b) {        // a * conj(b)
  return make_float2(fmaf(a.x, b.x, a.y * b.y), fmaf(a.y, b.x, -a.x * b.y));
}
// |X| from |X|^2: v_sqrt_f32 (1 ulp).  sqrtf() is the correctly rounded expansion - a scale test, the instruction, a one-ulp
// correction in both directions, the scaling back: sixteen instructions, four times per pair of bins (a quarter of the per-bin
// part of the loss kernels).  The instruction flushes denormal |X|^2: a bin below 1e-19 in magnitude counts as silent.
__device__ __forceinline__ float sl_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
// log2 (v_log_f32, 1 ulp) where only differences of logarithms are summed: the block's sum is scaled by ln 2 once, in fp64.
// __logf() is the accurate expansion - a denormal scale test, the instruction, an extended-precision product with ln 2, an
// infinity test: twelve instructions, four times per pair of bins.  Arguments here are >= safe_eps or normal magnitudes.
__device__ __forceinline__ float sl_log2(float x) { return __builtin_amdgcn_logf(x); }
constexpr double kSlLn2 = 0.6931471805599453;
__device__ __forceinline__ float2 sl_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 sl_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 sl_conj(float2 a) { return make_float2(a.x, -a.y); }

// frames g_lo .. g_lo + n_fr - 1 (H points each) of the array s.  The stage with q = 1 - the last of the forward transform, the
// first of the inverse - has unit twiddles: its instance (UNITY) neither makes nor multiplies by them.
template <int H, bool UNITY>
__device__ __forceinline__ void sl_fwd_stage8(float2* s, int tid, int n_fr, int g_lo, int q) {
  constexpr int LOG2H = SlPlan<H>::L;
  const float inv_len = 0.125f / (float)q;
  for (int t = tid; t < n_fr * (H / 8); t += kSlThreads) {
    const int g = t / (H / 8) + g_lo, r = t & (H / 8 - 1);
    const int pos = UNITY ? 0 : (r & (q - 1));
    const int i0 = (g << LOG2H) + ((r - pos) << 3) + pos;
    float2 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = s[SP(i0 + j * q)];
    fft_dft8(v);
    if constexpr (UNITY) {
#pragma unroll
      for (int m = 0; m < 8; ++m) s[SP(i0 + m * q)] = v[m];
    } else {
      float2 w[8];
      const float rev = (float)pos * inv_len;
      fft_powers8(make_float2(__builtin_amdgcn_cosf(rev), __builtin_amdgcn_sinf(rev)), w);   // conj of the twiddles
      s[SP(i0)] = v[0];
#pragma unroll
      for (int m = 1; m < 8; ++m) s[SP(i0 + m * q)] = sl_cmulc(v[m], w[m]);
    }
  }
  sl_stage_sync<H>();
}

template <int H, bool UNITY>
__device__ __forceinline__ void sl_fwd_stage4(float2* s, int tid, int n_fr, int g_lo, int q) {
  constexpr int LOG2H = SlPlan<H>::L;
  const float inv_len = 0.25f / (float)q;
  for (int t2 = 2 * tid; t2 < n_fr * (H / 4); t2 += 2 * kSlThreads) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = t2 + u;
      const int g = t / (H / 4) + g_lo, r = t & (H / 4 - 1);
      const int pos = UNITY ? 0 : (r & (q - 1));
      const int i0 = (g << LOG2H) + ((r - pos) << 2) + pos;
      const float2 a = s[SP(i0)], b = s[SP(i0 + q)], c = s[SP(i0 + 2 * q)], d = s[SP(i0 + 3 * q)];
      const float2 t0 = make_float2(a.x + c.x, a.y + c.y), t1 = make_float2(a.x - c.x, a.y - c.y);
      const float2 tb = make_float2(b.x + d.x, b.y + d.y), bd = make_float2(b.x - d.x, b.y - d.y);
      const float2 t3 = make_float2(bd.y, -bd.x);              // (b - d) * (-i)
      const float2 y0 = make_float2(t0.x + tb.x, t0.y + tb.y), y1 = make_float2(t1.x + t3.x, t1.y + t3.y),
                   y2 = make_float2(t0.x - tb.x, t0.y - tb.y), y3 = make_float2(t1.x - t3.x, t1.y - t3.y);
      s[SP(i0)] = y0;
      if constexpr (UNITY) {
        s[SP(i0 + q)] = y1; s[SP(i0 + 2 * q)] = y2; s[SP(i0 + 3 * q)] = y3;
      } else {
        const float rev = (float)pos * inv_len;
        const float2 w1 = make_float2(__builtin_amdgcn_cosf(rev), __builtin_amdgcn_sinf(rev));
        const float2 w2 = sl_cmul(w1, w1), w3 = sl_cmul(w2, w1);
        s[SP(i0 + q)] = sl_cmulc(y1, w1);
        s[SP(i0 + 2 * q)] = sl_cmulc(y2, w2);
        s[SP(i0 + 3 * q)] = sl_cmulc(y3, w3);
      }
    }
  }
  sl_stage_sync<H>();
}

// kSlFusedFirst<H>: the first stage of the forward transform is a radix-8 stage with twiddles (every H >= 32), which
// sl_load_stage1 runs on the samples as they arrive from memory; sl_forward<H, true> is the rest of the transform.
template <int H>
constexpr bool kSlFusedFirst = SlPlan<H>::N8 > 0 && (H / 8 > 1) && (H / 8 >= SlPlan<H>::M);

template <int H, bool SKIP_FIRST = false>
__device__ __forceinline__ void sl_forward(float2* s, int tid, int n_fr, int g_lo) {
  typedef SlPlan<H> P;
  if constexpr (P::N8 > 0) {
#pragma unroll 1
    for (int q = SKIP_FIRST ? H / 64 : H / 8; q >= P::M && q > 1; q >>= 3) sl_fwd_stage8<H, false>(s, tid, n_fr, g_lo, q);      // sub-length 8 q: H, H / 8, ..
    if constexpr (P::M == 1) sl_fwd_stage8<H, true>(s, tid, n_fr, g_lo, 1);
  }
  if constexpr (P::N4 > 0) {
#pragma unroll 1
    for (int q = P::M / 4; q > 1; q >>= 2) sl_fwd_stage4<H, false>(s, tid, n_fr, g_lo, q);
    sl_fwd_stage4<H, true>(s, tid, n_fr, g_lo, 1);
  }
}

template <int H, bool UNITY>
__device__ __forceinline__ void sl_inv_stage4(float2* s, int tid, int n_fr, int g_lo, int q) {
  constexpr int LOG2H = SlPlan<H>::L;
  const float inv_len = 0.25f / (float)q;
  for (int t2 = 2 * tid; t2 < n_fr * (H / 4); t2 += 2 * kSlThreads) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = t2 + u;
      const int g = t / (H / 4) + g_lo, r = t & (H / 4 - 1);
      const int pos = UNITY ? 0 : (r & (q - 1));
      const int i0 = (g << LOG2H) + ((r - pos) << 2) + pos;
      float2 y0 = s[SP(i0)], y1 = s[SP(i0 + q)], y2 = s[SP(i0 + 2 * q)], y3 = s[SP(i0 + 3 * q)];
      if constexpr (!UNITY) {
        const float rev = (float)pos * inv_len;
        const float2 w1 = make_float2(__builtin_amdgcn_cosf(rev), __builtin_amdgcn_sinf(rev));
        const float2 w2 = sl_cmul(w1, w1), w3 = sl_cmul(w2, w1);
        y1 = sl_cmul(y1, w1); y2 = sl_cmul(y2, w2); y3 = sl_cmul(y3, w3);
      }
      const float2 t0 = make_float2(y0.x + y2.x, y0.y + y2.y), tc = make_float2(y0.x - y2.x, y0.y - y2.y);
      const float2 t1 = make_float2(y1.x + y3.x, y1.y + y3.y), t3 = make_float2(y1.x - y3.x, y1.y - y3.y);
      const float2 bd = make_float2(-t3.y, t3.x);              // t3 * (+i)
      s[SP(i0)] = make_float2(t0.x + t1.x, t0.y + t1.y);
      s[SP(i0 + 2 * q)] = make_float2(t0.x - t1.x, t0.y - t1.y);
      s[SP(i0 + q)] = make_float2(tc.x + bd.x, tc.y + bd.y);
      s[SP(i0 + 3 * q)] = make_float2(tc.x - bd.x, tc.y - bd.y);
    }
  }
  sl_stage_sync<H>();
}

template <int H, bool UNITY>
__device__ __forceinline__ void sl_inv_stage8(float2* s, int tid, int n_fr, int g_lo, int q) {
  constexpr int LOG2H = SlPlan<H>::L;
  const float inv_len = 0.125f / (float)q;
  for (int t = tid; t < n_fr * (H / 8); t += kSlThreads) {
    const int g = t / (H / 8) + g_lo, r = t & (H / 8 - 1);
    const int pos = UNITY ? 0 : (r & (q - 1));
    const int i0 = (g << LOG2H) + ((r - pos) << 3) + pos;
    float2 v[8];
    // undo y_m conj(w^m), then the conjugate transform: sum_m y_m exp(+2 pi i j m / 8) = conj(dft8(conj y))
    if constexpr (UNITY) {
#pragma unroll
      for (int m = 0; m < 8; ++m) v[m] = sl_conj(s[SP(i0 + m * q)]);
    } else {
      float2 w[8];
      const float rev = (float)pos * inv_len;
      fft_powers8(make_float2(__builtin_amdgcn_cosf(rev), __builtin_amdgcn_sinf(rev)), w);
      v[0] = sl_conj(s[SP(i0)]);
#pragma unroll
      for (int m = 1; m < 8; ++m) v[m] = sl_conj(sl_cmul(s[SP(i0 + m * q)], w[m]));
    }
    fft_dft8(v);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[SP(i0 + j * q)] = sl_conj(v[j]);
  }
  sl_stage_sync<H>();
}

template <int H>
__device__ __forceinline__ void sl_inverse(float2* s, int tid, int n_fr, int g_lo) {
  typedef SlPlan<H> P;
  if constexpr (P::N4 > 0) {
    sl_inv_stage4<H, true>(s, tid, n_fr, g_lo, 1);
#pragma unroll 1
    for (int q = 4; q <= P::M / 4; q <<= 2) sl_inv_stage4<H, false>(s, tid, n_fr, g_lo, q);
  }
  if constexpr (P::N8 > 0) {
    if constexpr (P::M == 1) sl_inv_stage8<H, true>(s, tid, n_fr, g_lo, 1);
#pragma unroll 1
    for (int q = (P::M == 1 ? 8 : P::M); q <= H / 8; q <<= 3) sl_inv_stage8<H, false>(s, tid, n_fr, g_lo, q);
  }
}

// tf.signal.hann_window (periodic, an even number of points) at i / S turns, as sin^2(pi i / S): the textbook 0.5 - 0.5 cos(2 pi i / S)
// cancels at the window's first samples (v_cos_f32 is good to 1.2e-7 ABSOLUTE: 6e-4 of the window at sample 17 of 4096 points;
// TensorFlow's own fp32 op order 8e-5), which is all a clip much shorter than its frame ever sees of the window - round 5's fuzz
// campaigns ended on loss values of 17-sample clips 3e-4 ... 5e-4 off exact arithmetic (profiles/r05_fuzz_seed31_failures.jsonl).
// The square has no cancellation: 2e-5 there, one transcendental and one multiply like the other form.
__device__ __forceinline__ float sl_hann(float turns) {
  const float h = __builtin_amdgcn_sinf(0.5f * turns);
  return h * h;
}

// frames -> LDS, windowed: w[i] = 0.5 - 0.5 cos(2 pi i / S) (tf.signal.hann_window, periodic); element e
// of the array is the sample pair (2n, 2n+1) of frame e / H (first G frames: target, then audio).
// For H <= 512 a thread meets the same pair index n in every pass: its two window values are computed once.
template <int S>
__device__ __forceinline__ void sl_load_frames(float2* s, const float* __restrict__ trow,
                                               const float* __restrict__ arow, int tid, int f0,
                                               int n_frames, int N) {
  constexpr int H = S / 2, G = kSlPoints / 2 / H, LOG2H = __builtin_ctz(H), HOP = S / 4;
  constexpr int kPer = kSlPoints / kSlThreads;                // elements per thread
  constexpr bool kFixed = (kSlThreads % H) == 0;
  // 8-byte loads when every sample pair is 8-byte aligned (pairs start at even sample indices)
  const bool vec = ((N & 1) == 0) && (((reinterpret_cast<uintptr_t>(trow) | reinterpret_cast<uintptr_t>(arow)) & 7) == 0);
  float2 v[kPer];
  // all loads first: issued back to back, one wait (a load-use chain per element cost ~10 us per block)
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = tid + kSlThreads * u;
    const int g2 = e >> LOG2H, n2 = (e & (H - 1)) * 2;       // g2 < G: target frame, else audio frame
    const int g = g2 >= G ? g2 - G : g2;
    const int n = (f0 + g) * HOP + n2;
    v[u] = make_float2(0.f, 0.f);
    if (f0 + g < n_frames && n < N) {
      const float* __restrict__ row = g2 >= G ? arow : trow;
      if (vec) {
        v[u] = *reinterpret_cast<const float2*>(row + n);    // n + 1 < N: N and n are even
      } else {
        v[u].x = row[n];
        if (n + 1 < N) v[u].y = row[n + 1];
      }
    }
  }
  float w0 = 0.f, w1 = 0.f;
  if (kFixed) {
    const int n2 = (tid & (H - 1)) * 2;
    w0 = sl_hann((float)n2 * (1.0f / (float)S));
    w1 = sl_hann((float)(n2 + 1) * (1.0f / (float)S));
  }
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = tid + kSlThreads * u;
    if (!kFixed) {
      const int n2 = (e & (H - 1)) * 2;
      w0 = sl_hann((float)n2 * (1.0f / (float)S));
      w1 = sl_hann((float)(n2 + 1) * (1.0f / (float)S));
    }
    s[SP(e)] = make_float2(v[u].x * w0, v[u].y * w1);
  }
}

// The same for frames of F < S samples every `hop` under a window of F points, zero-padded to the transform's S (round 6: frames of
// 3 * 2^k samples - gin/models/vst/vst_48k.gin:56 - on the fused loss kernels; tf.signal.stft with fft_length=None transforms the
// enclosing power of two).  F is even: a sample pair is inside the frame or outside.
template <int S>
__device__ __forceinline__ void sl_load_frames_geom(float2* s, const float* __restrict__ trow, const float* __restrict__ arow, int tid,
                                                    int f0, int n_frames, int N, int F, int hop) {
  constexpr int H = S / 2, G = kSlPoints / 2 / H, LOG2H = __builtin_ctz(H);
  constexpr int kPer = kSlPoints / kSlThreads;
  const float inv_F = 1.0f / (float)F;
  float2 v[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = tid + kSlThreads * u;
    const int g2 = e >> LOG2H, n2 = (e & (H - 1)) * 2;
    const int g = g2 >= G ? g2 - G : g2;
    const long n = (long)(f0 + g) * hop + n2;
    v[u] = make_float2(0.f, 0.f);
    if (f0 + g < n_frames && n2 < F && n < N) {
      const float* __restrict__ row = g2 >= G ? arow : trow;
      v[u].x = row[n];
      if (n + 1 < N) v[u].y = row[n + 1];
    }
  }
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = tid + kSlThreads * u;
    const int n2 = (e & (H - 1)) * 2;
    s[SP(e)] = make_float2(v[u].x * sl_hann((float)n2 * inv_F), v[u].y * sl_hann((float)(n2 + 1) * inv_F));
  }
}

// Frames -> first radix-8 stage -> LDS (late round 5).  The first stage of the forward transform (q = H / 8) takes the
// elements r + j H / 8 (j = 0 .. 7) of a frame - with 2 G frames of H points and 512 threads exactly one butterfly per thread -
// so a thread can fetch those eight sample pairs itself, window them and write the stage's OUTPUT: the array is neither
// written by a load pass nor read back by the first stage (8 of a thread's 8 + 8 stages ds_write_b64, the expensive half of
// the LDS traffic - a 64-bit store occupies the store path for six cycles, a load the array for two), and one block barrier
// goes.  The window at those elements is cos(a + j / 8 turn): one sine and one cosine per sample parity give all sixteen
// values.  Frames past the end and samples past N are zeros, as in sl_load_frames.
template <int S>
__device__ __forceinline__ void sl_load_stage1(float2* s, const float* __restrict__ trow, const float* __restrict__ arow, int tid,
                                               int f0, int n_frames, int N) {
  constexpr int H = S / 2, G = kSlPoints / 2 / H, LOG2H = __builtin_ctz(H), HOP = S / 4, Q = H / 8;
  static_assert(2 * G * Q == kSlThreads, "one butterfly of the first stage per thread");
  const int g2 = tid / Q, r = tid & (Q - 1);
  const int g = g2 >= G ? g2 - G : g2;
  const float* __restrict__ row = g2 >= G ? arow : trow;
  const bool vec = ((N & 1) == 0) && (((reinterpret_cast<uintptr_t>(trow) | reinterpret_cast<uintptr_t>(arow)) & 7) == 0);
  const int n0 = (f0 + g) * HOP + 2 * r;
  const bool live = f0 + g < n_frames;
  float2 v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int n = n0 + j * (S / 8);
    v[j] = make_float2(0.f, 0.f);
    if (live && n < N) {
      if (vec) {
        v[j] = *reinterpret_cast<const float2*>(row + n);
      } else {
        v[j].x = row[n];
        if (n + 1 < N) v[j].y = row[n + 1];
      }
    }
  }
  // w[i] = 0.5 - 0.5 cos(2 pi i / S) at i = 2 r + j S / 8 (+ 1): cos(a + j pi / 4)
  const float kR = 0.70710678118654752f;
  const float a0 = (float)(2 * r) * (1.0f / (float)S), a1 = (float)(2 * r + 1) * (1.0f / (float)S);
  const float c0 = 0.5f * __builtin_amdgcn_cosf(a0), s0 = 0.5f * __builtin_amdgcn_sinf(a0);
  const float c1 = 0.5f * __builtin_amdgcn_cosf(a1), s1 = 0.5f * __builtin_amdgcn_sinf(a1);
  const float d0 = (c0 - s0) * kR, e0 = (c0 + s0) * kR, d1 = (c1 - s1) * kR, e1 = (c1 + s1) * kR;
  const float hc0[8] = {c0, d0, -s0, -e0, -c0, -d0, s0, e0};            // 0.5 cos(a0 + j pi / 4)
  const float hc1[8] = {c1, d1, -s1, -e1, -c1, -d1, s1, e1};
  // (j = 0 - the window's first eighth, where 0.5 - 0.5 cos cancels - as the square: sl_hann)
  v[0] = make_float2(v[0].x * sl_hann(a0), v[0].y * sl_hann(a1));
#pragma unroll
  for (int j = 1; j < 8; ++j) v[j] = make_float2(v[j].x * (0.5f - hc0[j]), v[j].y * (0.5f - hc1[j]));
  fft_dft8(v);
  float2 w[8];
  const float rev = (float)r * (0.125f / (float)Q);
  fft_powers8(make_float2(__builtin_amdgcn_cosf(rev), __builtin_amdgcn_sinf(rev)), w);   // conj of the twiddles
  const int i0 = (g2 << LOG2H) + r;
  s[SP(i0)] = v[0];
#pragma unroll
  for (int m = 1; m < 8; ++m) s[SP(i0 + m * Q)] = sl_cmulc(v[m], w[m]);
  sl_stage_sync<H>();
}

// frames of both signals, windowed and transformed (bin k at sl_pos<H>(k))
template <int S>
__device__ __forceinline__ void sl_frames_to_spectra(float2* s, const float* __restrict__ trow, const float* __restrict__ arow,
                                                     int tid, int f0, int n_frames, int N, int F = S, int hop = S / 4) {
  constexpr int H = S / 2, G = kSlPoints / 2 / H;
  if (F != S) {                          // (block-uniform) frames shorter than their transform: the plain load, then every stage
    sl_load_frames_geom<S>(s, trow, arow, tid, f0, n_frames, N, F, hop);
    __syncthreads();
    sl_forward<H>(s, tid, 2 * G, 0);
    if (SlPlan<H>::kWaveLocal) __syncthreads();
    return;
  }
  if constexpr (kSlFusedFirst<H>) {
    sl_load_stage1<S>(s, trow, arow, tid, f0, n_frames, N);
    sl_forward<H, true>(s, tid, 2 * G, 0);
  } else {
    sl_load_frames<S>(s, trow, arow, tid, f0, n_frames, N);
    __syncthreads();
    sl_forward<H>(s, tid, 2 * G, 0);
  }
  if (SlPlan<H>::kWaveLocal) __syncthreads();                  // the bins of a frame are read by other wavefronts
}

// One block of one FFT size: G frames of row b from frame bx * G on; nbx = blocks per row of this size.
template <int S>
__device__ __forceinline__ void stft_l1_block(float2* s, double (*red)[kSlThreads / 64], const float* __restrict__ target,
                                              const float* __restrict__ audio, double* __restrict__ partial, int N,
                                              int n_frames, float safe_eps, int bx, int b, int nbx, int F = S, int hop = S / 4) {
  // A real frame x[0..S) is transformed as the complex sequence z[n] = x[2n] + i x[2n+1] of H = S/2
  // points; X[k] = E[k] + exp(-2 pi i k / S) O[k] with E, O untangled from Z[k] and Z[H-k].  An
  // all-zero frame still gives exact zeros (nothing of another frame or signal is mixed in).
  constexpr int H = S / 2;
  constexpr int G = kSlPoints / 2 / H;  // frames per block (of each signal)
  constexpr int LOG2H = __builtin_ctz(H);
  const int tid = threadIdx.x;
  const int f0 = bx * G;
  const float* __restrict__ trow = target + (size_t)b * N;
  const float* __restrict__ arow = audio + (size_t)b * N;
  sl_frames_to_spectra<S>(s, trow, arow, tid, f0, n_frames, N, F, hop);
  // ---- untangle, magnitudes of bins 0 .. S/2, L1 terms ---------------------------------------------
  // per PAIR of bins (k, S/2 - k), k = 0 .. S/4: the two share the packed bins Z[k] and Z[H-k], their positions and the
  // twiddle (X[k] = E + W^k O, X[H-k] = conj(E - W^k O)) - half the LDS reads, bit reversals and sin / cos of a loop over
  // single bins (round 3: 156 instructions per bin were 30-45 % of this kernel)
  float dm = 0.0f, dl = 0.0f;
  // (k = 0 .. S/4 - 1 are G S/4 pairs - 1024 per block, two full trips of the 512 threads; the self-paired bin S/4 of
  // each frame goes in a short trip of its own: with it in the same loop - S/4 + 1 entries per frame - every size made
  // three trips for 2.004 .. 2.125 trips' worth of pairs, a third of this part of the kernel for nothing)
  auto pair_of_bins = [&](int g, int k, auto self_tag) {
    constexpr bool SELF = decltype(self_tag)::value;           // k = S/4: Z[k] pairs with itself, one bin
    const int ia = sl_pos<H>(k), ib = sl_pos<H>((H - k) & (H - 1));
    const float rev = (float)k * (1.0f / (float)S);
    const float c = __builtin_amdgcn_cosf(rev), sn = __builtin_amdgcn_sinf(rev);
    float m1[2], m2[2];
#pragma unroll
    for (int sig = 0; sig < 2; ++sig) {
      const int base = (g + sig * G) << LOG2H;
      const float2 za = s[SP(base + ia)], zb = s[SP(base + ib)];
      const float ex = 0.5f * (za.x + zb.x), ey = 0.5f * (za.y - zb.y);       // E = (Za + conj Zb) / 2
      const float ox = 0.5f * (za.y + zb.y), oy = -0.5f * (za.x - zb.x);      // O = (Za - conj Zb) / 2i
      const float wx = fmaf(ox, c, oy * sn), wy = fmaf(oy, c, -ox * sn);      // W^k O = (c - i sn) O
      const float x1r = ex + wx, x1i = ey + wy, x2r = ex - wx, x2i = ey - wy;
      m1[sig] = sl_sqrt(fmaf(x1r, x1r, x1i * x1i));                           // |X[k]|
      m2[sig] = sl_sqrt(fmaf(x2r, x2r, x2i * x2i));                           // |X[S/2 - k]|
    }
    dm += fabsf(m1[0] - m1[1]);
    // core.safe_log (core.py:213-216): non-positive -> eps
    dl += fabsf(sl_log2(m1[0] <= 0.0f ? safe_eps : m1[0]) - sl_log2(m1[1] <= 0.0f ? safe_eps : m1[1]));
    if (!SELF) {
      dm += fabsf(m2[0] - m2[1]);
      dl += fabsf(sl_log2(m2[0] <= 0.0f ? safe_eps : m2[0]) - sl_log2(m2[1] <= 0.0f ? safe_eps : m2[1]));
    }
  };
  constexpr int LOG2Q = LOG2H - 1;                             // pairs per frame in the main loop: H / 2
  for (int e = tid; e < G * (H / 2); e += kSlThreads) {
    const int g = e >> LOG2Q, k = e & (H / 2 - 1);
    if (f0 + g < n_frames) pair_of_bins(g, k, std::false_type{});
  }
  for (int g = tid; g < G; g += kSlThreads)
    if (f0 + g < n_frames) pair_of_bins(g, H / 2, std::true_type{});
  const double sm = (double)wave_sum(dm), sl = (double)wave_sum(dl);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sm; red[1][tid >> 6] = sl; }
  __syncthreads();
  if (tid == 0) {
    double a0 = 0.0, a1 = 0.0;
    for (int w = 0; w < kSlThreads / 64; ++w) { a0 += red[0][w]; a1 += red[1][w]; }
    double* out = partial + 2 * ((size_t)b * nbx + bx);
    out[0] = a0; out[1] = a1 * kSlLn2;            // (the log terms were summed in base 2)
  }
}

// Every FFT size of the loss in ONE launch (round 3): a size alone is 2016 blocks at batch 32 - two rounds of four blocks
// per CU that load, transform and reduce in step, six launches one after the other, each with its own ramp and tail; as one
// grid (the large sizes first) the blocks of different sizes and phases share the CUs.
struct SlMulti {
  int n;
  int size[16], first[17], nbx[16], frames[16], offset[16];      // per size: S, first linear block, blocks per row, frames, partial offset
  int frame[16];                                                 // ... and the frame's length F <= S (F < S: 3 * 2^k samples under 2^(k+2) points)
  FastDiv hop_div[16];                                           // F / 4
  float mag_scale[16], log_scale[16];                            // (the gradient kernel: weight / count of the size)
  int units;                                                     // > 0: the XCD-aware block order below (B * nbx units of n blocks)
  FastDiv n_div, nbx_div;                                        // n; nbx (the same for every size)
};
// WHICH block does what (late round 5).  Block bx of EVERY size starts at sample 1024 bx of its row (G frames of hop S / 4)
// and reads 1024 + 3 S / 4 samples of both signals from there: the n blocks (one per size) of a UNIT (row, bx) read the same
// 2 x 10 KB, and neighbouring units overlap by up to 1536 samples.  In the order "every block of size 2048, then every block
// of size 1024, .." a sample's 24 readers are spread over the whole launch and over the eight XCDs (block i runs on XCD
// i % 8, each with an L2 of its own: MI355X_MICROARCH.md, "Workgroup dispatch"): the L2s fetched 4.4 - 8.7 times the two
// signals' bytes through the fabric (profiles/r05g_*: FETCH_SIZE 286 MB a launch at batch 128 against 65.5 MB of input).
// Here XCD x = block % 8 owns a CONTIGUOUS eighth of the units and walks it in order, the n sizes of a unit side by side:
// what a block reads was read by its neighbours on the same L2 moments before.  Only the order of the blocks changes -
// a block's work and the slot its partial sums go to are the same, so the loss keeps its bits.
__device__ __forceinline__ bool sl_where(const SlMulti& m, int blk, int& z, int& b, int& bx) {
  if (m.units > 0) {
    const int x = blk & 7, q = blk >> 3;
    uint32_t rz, rbx;
    const int u = (int)fastdiv((uint32_t)q, m.n_div, rz);
    z = (int)rz;
    const int lo = (int)(((long long)x * m.units) >> 3), hi = (int)(((long long)(x + 1) * m.units) >> 3);
    const int unit = lo + u;
    if (unit >= hi) return false;
    b = (int)fastdiv((uint32_t)unit, m.nbx_div, rbx);
    bx = (int)rbx;
    return true;
  }
  z = 0;
  while (z + 1 < m.n && blk >= m.first[z + 1]) ++z;
  const int local = blk - m.first[z], nbx = m.nbx[z];
  b = local / nbx;
  bx = local - b * nbx;
  return true;
}

// ---- backward: dL/d audio ---------------------------------------------------------------------------
// Same block structure as the forward kernel: frames -> LDS -> forward FFT of target and audio frames.
// Then, per frame and per PAIR of bins (k, S/2-k) - the pair shares the packed bins Z[k], Z[H-k]:
//   magnitudes as forward -> dL/d|X_a| = -(w_mag sign(d mag) + w_log sign(d log) / |X_a|) / count
//   -> dL/dX_a = that * X_a / |X_a| -> the real-signal spectrum C of the frame's gradient
//   (C_0, C_{S/2} real parts, C_k = G_k / 2) -> re-packed into the H-point spectrum Z' (in place);
// an unscaled inverse FFT (the algebraic inverse of the forward stages) returns the frame's gradient
// as even/odd samples, which are windowed and added into grad_audio (4 overlapping frames per
// sample: fp32 atomics, so the last bit may differ from run to run).
// SLAB (the opt-in reproducible gradient; the order contract is stated above sl_grad_gather_kernel): a compile-time variant of the
// epilogue.  `grad_audio` is then the first float of this SCALE's slabs; block (b, bx) owns the (G + 3) hop floats
// [(b nbx + bx) (G + 3) hop ..) and STORES what the atomic instance adds, at the in-stretch index - sample f0 hop + p at index p.
// Every index whose sample lies in [0, N) is written (0 where no live frame covers it); the indices past the row's end are left
// as they are and the gather never reads them.  The atomic instances (SLAB = false) keep their instruction stream.
// COT (the general form of the loss, csrc/spectral_terms.hip): dL/d|X_a| is read from `cot` [B, frames, S/2+1] instead
// of being formed from the two spectra here; `target` is not looked at (the caller passes `audio` for it).
// One block of one FFT size (frames bx G .. of row b; nbx = blocks per row of this size).
template <int S, bool COT, bool SLAB = false>
__device__ __forceinline__ void stft_l1_bwd_block(float2* s, double (*red)[kSlThreads / 64], const float* __restrict__ target,
                                                  const float* __restrict__ audio, const float* __restrict__ grad_loss,
                                                  float* __restrict__ grad_audio, int N, int n_frames, float safe_eps,
                                                  float mag_scale, float log_scale, double* __restrict__ partial,
                                                  const float* __restrict__ cot, int bx, int b, int nbx, int F = S,
                                                  FastDiv hop_div = FastDiv{(uint32_t)(S / 4), 0u}) {
  constexpr int H = S / 2;
  constexpr int G = kSlPoints / 2 / H;
  constexpr int LOG2H = __builtin_ctz(H);
  constexpr int HOP = S / 4;
  const int tid = threadIdx.x;
  const int f0 = bx * G;
  const float* __restrict__ trow = target + (size_t)b * N;
  const float* __restrict__ arow = audio + (size_t)b * N;
  sl_frames_to_spectra<S>(s, trow, arow, tid, f0, n_frames, N, F, (int)hop_div.d);
  // ---- bins -> gradient spectrum, in place in the audio half of the array --------------------------
  // grad_loss == nullptr: the fused loss + gradient call - dL/dloss = 1 and the block's L1 sums go to
  // `partial` exactly as stft_l1_kernel writes them (the frame spectra are computed once for both)
  const float up = grad_loss ? grad_loss[0] : 1.0f;
  const float ms = mag_scale * up, ls = log_scale * up;        // weight / count (per size), times dL/dloss
  float dm_sum = 0.0f, dl_sum = 0.0f;
  // (pairs k = 0 .. H/2 - 1 in two full trips of the block, the self-paired bin H/2 of every frame in a short trip of its
  // own: as in stft_l1_block)
  auto pair_grad = [&](int g, int k) {                          // pair (k, H-k)
    const int ia = sl_pos<H>(k), ib = sl_pos<H>((H - k) & (H - 1));
    const float rev = (float)k * (1.0f / (float)S);
    const float c = __builtin_amdgcn_cosf(rev), sn = __builtin_amdgcn_sinf(rev);
    float2 x1[2], x2[2];                                        // X[k], X[H-k] of target (0) and audio (1)
#pragma unroll
    for (int sig = 0; sig < 2; ++sig) {
      const int base = (g + sig * G) << LOG2H;
      const float2 za = s[SP(base + ia)], zb = s[SP(base + ib)];
      const float ex = 0.5f * (za.x + zb.x), ey = 0.5f * (za.y - zb.y);
      const float ox = 0.5f * (za.y + zb.y), oy = -0.5f * (za.x - zb.x);
      const float wx = fmaf(ox, c, oy * sn), wy = fmaf(oy, c, -ox * sn);     // W^k O
      x1[sig] = make_float2(ex + wx, ey + wy);                  // X[k]   = E + W^k O
      x2[sig] = make_float2(ex - wx, -(ey - wy));               // X[H-k] = conj(E - W^k O)
    }
    // dL/dX for one bin: coefficient * X_a / |X_a|
    auto bin_grad = [&](float2 xt, float2 xa, bool count, int bin) {
      if constexpr (COT) {
        const float ma = sl_sqrt(fmaf(xa.x, xa.x, xa.y * xa.y));
        if (ma <= 0.0f) return make_float2(0.f, 0.f);             // |z| has gradient 0 at z = 0 (tf.abs); a NaN |z| is no zero
        const float coef = cot[((size_t)b * n_frames + f0 + g) * (H + 1) + bin] * __builtin_amdgcn_rcpf(ma);
        return make_float2(coef * xa.x, coef * xa.y);
      }
      const float mt = sl_sqrt(fmaf(xt.x, xt.x, xt.y * xt.y)), ma = sl_sqrt(fmaf(xa.x, xa.x, xa.y * xa.y));
      if (count) {                                              // every bin 0 .. S/2 exactly once
        dm_sum += fabsf(mt - ma);
        dl_sum += fabsf(sl_log2(mt <= 0.0f ? safe_eps : mt) - sl_log2(ma <= 0.0f ? safe_eps : ma));
      }
      if (ma <= 0.0f) return make_float2(0.f, 0.f);
      const float dmag = mt - ma;
      const float dlog = sl_log2(mt <= 0.0f ? safe_eps : mt) - sl_log2(ma);
      const float sm = dmag > 0.0f ? 1.0f : (dmag < 0.0f ? -1.0f : 0.0f);
      const float sl = dlog > 0.0f ? 1.0f : (dlog < 0.0f ? -1.0f : 0.0f);
      const float inv = __builtin_amdgcn_rcpf(ma);
      const float coef = -(ms * sm + ls * sl * inv) * inv;
      return make_float2(coef * xa.x, coef * xa.y);
    };
    float2 c1 = bin_grad(x1[0], x1[1], true, k);                // G[k]
    float2 c2 = bin_grad(x2[0], x2[1], 2 * k != H, H - k);      // G[H-k] (the self-paired bin S/4 counts once)
    const int abase = (g + G) << LOG2H;
    if (k == 0) {                                               // bins 0 and S/2: real, C = Re G
      const float e0 = 0.5f * (c1.x + c2.x), o0 = 0.5f * (c1.x - c2.x);
      s[SP(abase + ia)] = make_float2(e0, o0);                      // Z'[0] = E' + i O'
    } else {
      if (2 * k == H) c2 = c1;                                  // the self-paired bin S/4
      c1 = make_float2(0.5f * c1.x, 0.5f * c1.y);               // C_k = G_k / 2 for inner bins
      c2 = make_float2(0.5f * c2.x, 0.5f * c2.y);
      // E' = (C[k] + conj C[H-k]) / 2,  O' = (C[k] - conj C[H-k]) / 2 * W^-k
      const float ex = 0.5f * (c1.x + c2.x), ey = 0.5f * (c1.y - c2.y);
      const float dx = 0.5f * (c1.x - c2.x), dy = 0.5f * (c1.y + c2.y);
      const float ox = fmaf(dx, c, -dy * sn), oy = fmaf(dx, sn, dy * c);      // D * (c + i sn)
      s[SP(abase + ia)] = make_float2(ex - oy, ey + ox);            // Z'[k]   = E' + i O'
      if (2 * k != H) s[SP(abase + ib)] = make_float2(ex + oy, ox - ey);          // Z'[H-k] = conj E' + i conj O'
    }
  };
  for (int e = tid; e < G * (H / 2); e += kSlThreads) {
    const int g = e >> (LOG2H - 1), k = e & (H / 2 - 1);
    if (f0 + g < n_frames) pair_grad(g, k);
  }
  for (int g = tid; g < G; g += kSlThreads)
    if (f0 + g < n_frames) pair_grad(g, H / 2);
  __syncthreads();
  // ---- unscaled inverse transform of the audio frames ------------------------------------------------
  sl_inverse<H>(s, tid, G, G);
  if (SlPlan<H>::kWaveLocal) __syncthreads();
  // ---- window and overlap-add: g_x[2n] = 2 Re U[n], g_x[2n+1] = 2 Im U[n] ------------------------------
  // Gathered per output sample: the (up to) four frames of this block that cover it are summed from
  // LDS first.  A sample whose four frames all belong to this block is owned by the block - plain
  // read-modify-write (the kernels of the other FFT sizes run before or after, never beside this
  // one); only the three hops at either end of the block's range are shared with the neighbouring
  // blocks and go through fp32 atomics.  (One atomic per frame and sample, 49 M per call at batch 32,
  // was the bound of this kernel.)
  float* __restrict__ grow = SLAB ? grad_audio + ((size_t)b * nbx + bx) * (size_t)((G + 3) * (int)hop_div.d)
                                  : grad_audio + (size_t)b * N;
  if (F != S) {
    // frames of F = 4 hop samples under a transform of S points (round 6): the same gather with the hop a run-time number - a
    // division by it (fastdiv) and the window by its own sine per frame
    const int hop = (int)hop_div.d;
    const float inv_F = 1.0f / (float)F;
    if ((hop & 1) == 0) {                                      // (every 3 * 2^k frame the fused path takes: hop = 3 * 2^(k - 2), k >= 4)
      // sample pairs, as below: four LDS reads per pair
      for (int pp = tid; pp < (G + 3) * (hop >> 1); pp += kSlThreads) {
        const int pidx = 2 * pp;
        const long n = (long)f0 * hop + pidx;
        if (n >= N) continue;
        uint32_t ir_;
        const int gp = (int)fastdiv((uint32_t)pidx, hop_div, ir_), ir = (int)ir_;       // (ir even)
        float acc0 = 0.0f, acc1 = 0.0f;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int g = gp - jj, i = ir + jj * hop;
          if (g >= 0 && g < G && f0 + g < n_frames) {
            const float2 u = s[SP(((g + G) << LOG2H) + (i >> 1))];
            acc0 = fmaf(2.0f * u.x, sl_hann((float)i * inv_F), acc0);
            acc1 = fmaf(2.0f * u.y, sl_hann((float)(i + 1) * inv_F), acc1);
          }
        }
        if constexpr (SLAB) {
          *reinterpret_cast<float2*>(&grow[pidx]) = make_float2(acc0, acc1);       // (pidx and the stretch are even: 8-byte aligned)
        } else {
        unsafeAtomicAdd(&grow[n], acc0);
        if (n + 1 < N) unsafeAtomicAdd(&grow[n + 1], acc1);
        }
      }
    } else
    for (int pidx = tid; pidx < (G + 3) * hop; pidx += kSlThreads) {
      const long n = (long)f0 * hop + pidx;
      if (n >= N) continue;
      uint32_t ir_;
      const int gp = (int)fastdiv((uint32_t)pidx, hop_div, ir_), ir = (int)ir_;
      float acc = 0.0f;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int g = gp - jj, i = ir + jj * hop;             // frame g covers the sample at its index i < F
        if (g >= 0 && g < G && f0 + g < n_frames) {
          const float2 u = s[SP(((g + G) << LOG2H) + (i >> 1))];
          acc = fmaf(2.0f * ((i & 1) ? u.y : u.x), sl_hann((float)i * inv_F), acc);
        }
      }
      if constexpr (SLAB) grow[pidx] = acc;
      else unsafeAtomicAdd(&grow[n], acc);
    }
  } else {
  constexpr int LOG2HOP = __builtin_ctz(HOP);
  // (round 6) a lane takes the sample PAIR (2 m, 2 m + 1): both sit in one element of the transform (Re, Im), so the four frames
  // that cover them cost four LDS reads per pair instead of eight - the same fused multiply-adds per sample in the same order
  static_assert((HOP & 1) == 0, "sample pairs do not straddle a hop");
  for (int pp = tid; pp < (G + 3) * (HOP / 2); pp += kSlThreads) {
    const int pidx = 2 * pp;
    const int n = f0 * HOP + pidx;
    if (n >= N) continue;
    const int gp = pidx >> LOG2HOP, ir = pidx & (HOP - 1);   // (ir even)
    float acc0 = 0.0f, acc1 = 0.0f;
    // the window at i = ir + jj S/4: cos(x + jj pi/2) = cos x, -sin x, -cos x, sin x - one sine and one cosine for the four frames
    const float wrev0 = (float)ir * (1.0f / (float)S), wrev1 = (float)(ir + 1) * (1.0f / (float)S);
    const float hc0 = 0.5f * __builtin_amdgcn_cosf(wrev0), hs0 = 0.5f * __builtin_amdgcn_sinf(wrev0);
    const float hc1 = 0.5f * __builtin_amdgcn_cosf(wrev1), hs1 = 0.5f * __builtin_amdgcn_sinf(wrev1);
    const float wj0[4] = {sl_hann(wrev0), 0.5f + hs0, 0.5f + hc0, 0.5f - hs0};      // (the first quarter as the square: sl_hann)
    const float wj1[4] = {sl_hann(wrev1), 0.5f + hs1, 0.5f + hc1, 0.5f - hs1};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int g = gp - jj, i = ir + jj * HOP;               // frame g covers the pair at its indices i, i + 1
      if (g >= 0 && g < G && f0 + g < n_frames) {
        const float2 u = s[SP(((g + G) << LOG2H) + (i >> 1))];
        acc0 = fmaf(2.0f * u.x, wj0[jj], acc0);
        acc1 = fmaf(2.0f * u.y, wj1[jj], acc1);
      }
    }
    // (one fp32 atomic per sample and block, every one of them: blocks of every FFT size run side by side since the end of
    // round 3.  Rounds 2-3 kept plain read-modify-writes for the samples a block owns among the blocks of ITS size - and
    // were no faster for it: 190 us against 182 with atomics throughout, profiles/r03v_*)
    if constexpr (SLAB) {
      *reinterpret_cast<float2*>(&grow[pidx]) = make_float2(acc0, acc1);
    } else {
    unsafeAtomicAdd(&grow[n], acc0);
    if (n + 1 < N) unsafeAtomicAdd(&grow[n + 1], acc1);
    }
  }
  }
  if (partial) {                                               // block-uniform
    const double sm = (double)wave_sum(dm_sum), sl = (double)wave_sum(dl_sum);
    if ((tid & 63) == 0) { red[0][tid >> 6] = sm; red[1][tid >> 6] = sl; }
    __syncthreads();
    if (tid == 0) {
      double a0 = 0.0, a1 = 0.0;
      for (int w = 0; w < kSlThreads / 64; ++w) { a0 += red[0][w]; a1 += red[1][w]; }
      double* out = partial + 2 * ((size_t)b * nbx + bx);
      out[0] = a0; out[1] = a1 * kSlLn2;            // (the log terms were summed in base 2)
    }
  }
}

// =====================================================================================================================
// Transforms of 8192 points on the fused 'L1' path (round 6, second half): frames of 8192 samples, and the 6144-sample frames
// gin/models/vst/vst_48k.gin:56 asks for (zero-padded to 8192 points, as tf.signal.stft does).  ONE frame of ONE signal fills a
// block's 4096 complex points, so a block takes the two signals in turn: the target frame is transformed first and only its
// magnitudes survive - eight and a bit per thread, in registers, which is all the loss and its gradient ever ask of the target
// (bin_grad above: X_t enters through |X_t| alone) -, then the audio frame goes through the same array; the gradient spectrum
// is formed in place, transformed back and overlap-added as in stft_l1_bwd_block.  Kernels of their own (stft_l1_big_kernel,
// stft_l1_big_bwd_kernel): the nine live registers across a transform and the 64-register budget that keeps four blocks of the
// other sizes on a CU do not go together.  Their partial sums land in the same buffer, the finish kernel is the same.
// (Until here such frames ran the plain kernels - magnitudes through HBM, a launch per term: vst_48k.gin's loss spent half its
// time on this one scale of six, profiles/r06_loss_vst48k_frame_sizes.json.)
// =====================================================================================================================
constexpr int kSlBigS = 8192;
// SLAB (BWD only): `grad_audio` is the first float of this scale's slabs; the block of frame f owns the F floats
// [(b n_frames + f) F ..) and stores sample f hop + i at index i (as stft_l1_bwd_block: every index whose sample lies inside
// the row is written, the rest is never read).
template <bool BWD, bool SLAB = false>
__device__ __forceinline__ void stft_l1_big_block(float2* s, double (*red)[kSlThreads / 64], const float* __restrict__ target,
                                                  const float* __restrict__ audio, const float* __restrict__ grad_loss,
                                                  float* __restrict__ grad_audio, int N, float safe_eps, float mag_scale,
                                                  float log_scale, double* __restrict__ partial, int f, int b, int n_frames, int F,
                                                  int hop) {
  constexpr int S = kSlBigS, H = S / 2, LOG2H = __builtin_ctz(H);
  constexpr int kPer = H / kSlThreads, kPairs = (H / 2) / kSlThreads;       // 8 elements, 4 bin pairs per thread
  static_assert(kPer * kSlThreads == H && kPairs * kSlThreads == H / 2, "one frame per block");
  static_assert(H <= kSlPoints, "the frame's complex points fit the array");
  (void)LOG2H;
  const int tid = threadIdx.x;
  const float inv_F = 1.0f / (float)F;
  const long n00 = (long)f * hop;
  // a frame of F samples (every hop) under a window of F points, zero-padded to S: elements e = sample pairs (2 e, 2 e + 1)
  auto load_frame = [&](const float* __restrict__ row) {
    float2 v[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int n2 = 2 * (tid + kSlThreads * u);
      const long n = n00 + n2;
      v[u] = make_float2(0.f, 0.f);
      if (n2 < F && n < N) {                                   // (F is even: the pair is inside the frame or outside)
        v[u].x = row[n];
        if (n + 1 < N) v[u].y = row[n + 1];
      }
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int e = tid + kSlThreads * u, n2 = 2 * e;
      s[SP(e)] = make_float2(v[u].x * sl_hann((float)n2 * inv_F), v[u].y * sl_hann((float)(n2 + 1) * inv_F));
    }
    __syncthreads();
    sl_forward<H>(s, tid, 1, 0);                               // (every stage ends in a block barrier: H / 8 > 64)
  };
  // X[k] and X[H - k] of the frame in the array (pair k; k = 0: bins 0 and S / 2)
  auto pair_spectrum = [&](int k, float c, float sn, float2& x1, float2& x2) {
    const int ia = sl_pos<H>(k), ib = sl_pos<H>((H - k) & (H - 1));
    const float2 za = s[SP(ia)], zb = s[SP(ib)];
    const float ex = 0.5f * (za.x + zb.x), ey = 0.5f * (za.y - zb.y);
    const float ox = 0.5f * (za.y + zb.y), oy = -0.5f * (za.x - zb.x);
    const float wx = fmaf(ox, c, oy * sn), wy = fmaf(oy, c, -ox * sn);       // W^k O
    x1 = make_float2(ex + wx, ey + wy);                        // X[k]   = E + W^k O
    x2 = make_float2(ex - wx, -(ey - wy));                     // X[H-k] = conj(E - W^k O)
  };
  auto mag = [](float2 x) { return sl_sqrt(fmaf(x.x, x.x, x.y * x.y)); };
  const float* __restrict__ trow = target + (size_t)b * N;
  const float* __restrict__ arow = audio + (size_t)b * N;
  const bool live = f < n_frames;                              // (block-uniform; the grid has one block per frame)
  // ---- the target frame: magnitudes into registers ----------------------------------------------------------------------
  float mt1[kPairs], mt2[kPairs], mts = 0.0f;
#pragma unroll
  for (int u = 0; u < kPairs; ++u) { mt1[u] = 0.0f; mt2[u] = 0.0f; }
  if (live) {
    load_frame(trow);
#pragma unroll
    for (int u = 0; u < kPairs; ++u) {
      const int k = tid + kSlThreads * u;
      const float rev = (float)k * (1.0f / (float)S);
      float2 x1, x2;
      pair_spectrum(k, __builtin_amdgcn_cosf(rev), __builtin_amdgcn_sinf(rev), x1, x2);
      mt1[u] = mag(x1); mt2[u] = mag(x2);
    }
    if (tid == 0) {
      float2 x1, x2;
      pair_spectrum(H / 2, __builtin_amdgcn_cosf(0.25f), __builtin_amdgcn_sinf(0.25f), x1, x2);
      mts = mag(x1);
    }
    __syncthreads();                                           // every thread has read the target's spectrum
    load_frame(arow);
  }
  // ---- the audio frame: the L1 sums, and (BWD) the gradient spectrum in place ----------------------------------------------
  const float up = (BWD && grad_loss) ? grad_loss[0] : 1.0f;
  const float ms = mag_scale * up, ls = log_scale * up;
  float dm_sum = 0.0f, dl_sum = 0.0f;
  auto bin_grad = [&](float mt, float2 xa, bool count) -> float2 {         // as stft_l1_bwd_block's, the target by its magnitude
    const float ma = mag(xa);
    const float lt = sl_log2(mt <= 0.0f ? safe_eps : mt), la = sl_log2(ma <= 0.0f ? safe_eps : ma);
    if (count) {
      dm_sum += fabsf(mt - ma);
      dl_sum += fabsf(lt - la);
    }
    if (!BWD || ma <= 0.0f) return make_float2(0.f, 0.f);
    const float dmag = mt - ma, dlog = lt - la;
    const float sm = dmag > 0.0f ? 1.0f : (dmag < 0.0f ? -1.0f : 0.0f);
    const float sl = dlog > 0.0f ? 1.0f : (dlog < 0.0f ? -1.0f : 0.0f);
    const float inv = __builtin_amdgcn_rcpf(ma);
    const float coef = -(ms * sm + ls * sl * inv) * inv;
    return make_float2(coef * xa.x, coef * xa.y);
  };
  auto pair_bins = [&](int k, float mta, float mtb) {
    const float rev = (float)k * (1.0f / (float)S);
    const float c = __builtin_amdgcn_cosf(rev), sn = __builtin_amdgcn_sinf(rev);
    float2 x1, x2;
    pair_spectrum(k, c, sn, x1, x2);
    float2 c1 = bin_grad(mta, x1, true);
    float2 c2 = bin_grad(mtb, x2, 2 * k != H);                 // (the self-paired bin S / 4 counts once)
    if constexpr (BWD) {
      const int ia = sl_pos<H>(k), ib = sl_pos<H>((H - k) & (H - 1));
      if (k == 0) {                                            // bins 0 and S / 2: real, C = Re G
        s[SP(ia)] = make_float2(0.5f * (c1.x + c2.x), 0.5f * (c1.x - c2.x));
      } else {
        if (2 * k == H) c2 = c1;
        c1 = make_float2(0.5f * c1.x, 0.5f * c1.y);            // C_k = G_k / 2 for inner bins
        c2 = make_float2(0.5f * c2.x, 0.5f * c2.y);
        const float ex = 0.5f * (c1.x + c2.x), ey = 0.5f * (c1.y - c2.y);
        const float dx = 0.5f * (c1.x - c2.x), dy = 0.5f * (c1.y + c2.y);
        const float ox = fmaf(dx, c, -dy * sn), oy = fmaf(dx, sn, dy * c);
        s[SP(ia)] = make_float2(ex - oy, ey + ox);             // Z'[k]   = E' + i O'
        if (2 * k != H) s[SP(ib)] = make_float2(ex + oy, ox - ey);          // Z'[H-k] = conj E' + i conj O'
      }
    }
  };
  if (live) {
#pragma unroll
    for (int u = 0; u < kPairs; ++u) pair_bins(tid + kSlThreads * u, mt1[u], mt2[u]);
    if (tid == 0) pair_bins(H / 2, mts, mts);
  }
  if constexpr (BWD) {
    if (live) {
      __syncthreads();
      sl_inverse<H>(s, tid, 1, 0);
      // window and overlap-add: sample i of the frame is element i / 2 of the transform, 2 Re / 2 Im (stft_l1_bwd_block); every
      // sample through an atomic (the three other frames that cover it belong to other blocks)
      float* __restrict__ grow = SLAB ? grad_audio + ((size_t)b * n_frames + f) * (size_t)F : grad_audio + (size_t)b * N;
      for (int i = tid; i < F; i += kSlThreads) {
        const long n = n00 + i;
        if (n >= N) break;
        const float2 u = s[SP(i >> 1)];
        if constexpr (SLAB) grow[i] = 2.0f * ((i & 1) ? u.y : u.x) * sl_hann((float)i * inv_F);
        else unsafeAtomicAdd(&grow[n], 2.0f * ((i & 1) ? u.y : u.x) * sl_hann((float)i * inv_F));
      }
    } else if constexpr (SLAB) {                             // (no such block in a grid of n_frames blocks; zeros if there were)
      float* __restrict__ grow = grad_audio + ((size_t)b * n_frames + f) * (size_t)F;
      for (int i = tid; i < F && n00 + i < N; i += kSlThreads) grow[i] = 0.0f;
    }
  }
  if (partial) {
    const double sm = (double)wave_sum(dm_sum), sl = (double)wave_sum(dl_sum);
    if ((tid & 63) == 0) { red[0][tid >> 6] = sm; red[1][tid >> 6] = sl; }
    __syncthreads();
    if (tid == 0) {
      double a0 = 0.0, a1 = 0.0;
      for (int w = 0; w < kSlThreads / 64; ++w) { a0 += red[0][w]; a1 += red[1][w]; }
      double* out = partial + 2 * ((size_t)b * n_frames + f);
      out[0] = a0; out[1] = a1 * kSlLn2;
    }
  }
}

// =====================================================================================================================
// Frame sizes 3 * 2^k (gin/models/vst/vst_48k.gin:56 asks for 6144, 3072, .. 192).  spectral_ops.stft (spectral_ops.py:34-47)
// calls tf.signal.stft with fft_length=None: frames of F samples every F / 4, a periodic Hann window of F points - and an FFT of
// the ENCLOSING POWER OF TWO S = 4 F / 3, the frame zero-padded to it: S / 2 + 1 bins.  So no radix-3 pass is needed; what
// differs from the kernels above is the frame (length, hop, window) under the same power-of-two transform.  Plain kernels for
// the general form of the loss (ddsp_stft_mag_f32 / ddsp_stft_mag_backward_f32 + csrc/spectral_terms.hip): one signal per
// block (the largest size - 6144 samples under an 8192-point transform - fills a block's 4096 complex points with ONE frame),
// a load pass of its own, every output sample through an atomic.
// =====================================================================================================================
// A frame geometry under a transform of S points: frames of F <= S samples (F even) every `hop`, the first starting `pad_left`
// samples BEFORE sample 0 (spectral_ops.pad 'center': F / 2), a periodic Hann window of F points, zeros up to S and outside the row.
//   vst_48k.gin's loss frames: F = 3 S / 4, hop F / 4, pad_left 0;  compute_loudness: F = S = 2048, hop 64, pad_left 1024.
struct SlFrameGeom { int F, hop, pad_left; float inv_F; };

// frames [f0, f0 + n_fr) of `row`: element e of frame g is the sample pair (2 e, 2 e + 1)
template <int S>
__device__ __forceinline__ void tq_load_frames(float2* s, const float* __restrict__ row, int tid, int f0, int n_fr,
                                               int n_frames, int N, SlFrameGeom fg) {
  constexpr int H = S / 2, LOG2H = __builtin_ctz(H);
  for (int it = tid; it < n_fr * H; it += kSlThreads) {
    const int g = it >> LOG2H, e = it & (H - 1);
    float x0 = 0.0f, x1 = 0.0f, w0 = 0.0f, w1 = 0.0f;
    if (f0 + g < n_frames && 2 * e < fg.F) {                     // (F is even: a pair is inside the frame or outside)
      const long i = (long)(f0 + g) * fg.hop - fg.pad_left + 2 * e;
      if (i >= 0 && i < N) x0 = row[i];
      if (i + 1 >= 0 && i + 1 < N) x1 = row[i + 1];
      // tf.signal.hann_window(F), periodic: 0.5 - 0.5 cos(2 pi i / F)
      w0 = sl_hann((float)(2 * e) * fg.inv_F);
      w1 = sl_hann((float)(2 * e + 1) * fg.inv_F);
    }
    s[SP(it)] = make_float2(x0 * w0, x1 * w1);
  }
}

// dL/d audio from dL/d |STFT(audio)| (`cot` [B, frames, S / 2 + 1]); stft_l1_bwd_block's arithmetic on frames of 3 S / 4 samples
// SLAB: `grad_audio` is the first float of the slabs; block (b, bx) owns the `span` floats [(b gridDim.x + bx) span ..) and stores
// position p of its stretch at index p (every p whose sample lies inside the row, 0 where no live frame covers it).
// (A kernel template, not a block function under two kernels: wrapped in a function, the atomic instances came out with their
// instructions in another order.  spectral_loss.hip instantiates SLAB = false, spectral_loss_det.hip SLAB = true.)
template <int S, bool SLAB = false>
__global__ __launch_bounds__(kSlThreads) void stft_tq_cot_bwd_kernel(const float* __restrict__ audio, float* __restrict__ grad_audio,
                                                                     int N, int n_frames, const float* __restrict__ cot,
                                                                     SlFrameGeom fg) {
  constexpr int H = S / 2, G = kSlPoints / H;
  __shared__ __attribute__((aligned(16))) float2 s[kSlStore];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int f0 = blockIdx.x * G;
  tq_load_frames<S>(s, audio + (size_t)b * N, tid, f0, G, n_frames, N, fg);
  __syncthreads();
  sl_forward<H>(s, tid, G, 0);
  __syncthreads();
  for (int e = tid; e < G * (H / 2 + 1); e += kSlThreads) {      // pairs of bins (k, H - k), k = 0 .. H / 2
    const int g = e / (H / 2 + 1), k = e - g * (H / 2 + 1);
    if (f0 + g >= n_frames) continue;
    const int pa = g * H + sl_pos<H>(k), pb = g * H + sl_pos<H>((H - k) & (H - 1));
    const float rev = (float)k * (1.0f / (float)S);
    const float c = __builtin_amdgcn_cosf(rev), sn = __builtin_amdgcn_sinf(rev);
    const float2 za = s[SP(pa)], zb = s[SP(pb)];
    const float ex = 0.5f * (za.x + zb.x), ey = 0.5f * (za.y - zb.y);
    const float ox = 0.5f * (za.y + zb.y), oy = -0.5f * (za.x - zb.x);
    const float wx = fmaf(ox, c, oy * sn), wy = fmaf(oy, c, -ox * sn);       // W^k O
    const float2 x1 = make_float2(ex + wx, ey + wy);                          // X[k]   = E + W^k O
    const float2 x2 = make_float2(ex - wx, -(ey - wy));                       // X[H-k] = conj(E - W^k O)
    const float* __restrict__ crow = cot + ((size_t)b * n_frames + f0 + g) * (H + 1);
    auto bin_grad = [&](float2 xa, int bin) {                                 // dL/dX: cot * X / |X| (0 at X = 0: tf.abs)
      const float ma = sl_sqrt(fmaf(xa.x, xa.x, xa.y * xa.y));
      if (ma <= 0.0f) return make_float2(0.f, 0.f);
      const float coef = crow[bin] * __builtin_amdgcn_rcpf(ma);
      return make_float2(coef * xa.x, coef * xa.y);
    };
    float2 c1 = bin_grad(x1, k), c2 = bin_grad(x2, H - k);
    if (k == 0) {                                               // bins 0 and S/2: real, C = Re G
      const float e0 = 0.5f * (c1.x + c2.x), o0 = 0.5f * (c1.x - c2.x);
      s[SP(pa)] = make_float2(e0, o0);
    } else {
      if (2 * k == H) c2 = c1;                                  // the self-paired bin S/4
      c1 = make_float2(0.5f * c1.x, 0.5f * c1.y);
      c2 = make_float2(0.5f * c2.x, 0.5f * c2.y);
      const float gx = 0.5f * (c1.x + c2.x), gy = 0.5f * (c1.y - c2.y);
      const float dx = 0.5f * (c1.x - c2.x), dy = 0.5f * (c1.y + c2.y);
      const float qx = fmaf(dx, c, -dy * sn), qy = fmaf(dx, sn, dy * c);      // D * (c + i sn)
      s[SP(pa)] = make_float2(gx - qy, gy + qx);
      if (2 * k != H) s[SP(pb)] = make_float2(gx + qy, qx - gy);
    }
  }
  __syncthreads();
  sl_inverse<H>(s, tid, G, 0);
  __syncthreads();
  // window and overlap-add: g_x[2 e] = 2 Re U[e], g_x[2 e + 1] = 2 Im U[e] for the frame's first F samples (the zero padding
  // has no gradient); position p of the block's stretch (sample f0 hop - pad_left + p) lies in frames g with 0 <= p - g hop < F
  float* __restrict__ grow = grad_audio + (SLAB ? ((size_t)b * gridDim.x + blockIdx.x) * (size_t)((G - 1) * fg.hop + fg.F) : (size_t)b * N);
  const int span = (G - 1) * fg.hop + fg.F;
  for (int p = tid; p < span; p += kSlThreads) {
    const long n = (long)f0 * fg.hop - fg.pad_left + p;
    if (n < 0 || n >= N) continue;
    const int g_hi = min(G - 1, p / fg.hop);
    const int g_lo = p < fg.F ? 0 : (p - fg.F) / fg.hop + 1;
    float acc = 0.0f;
    for (int g = g_lo; g <= g_hi; ++g) {
      if (f0 + g >= n_frames) break;
      const int i = p - g * fg.hop;                              // < F
      const float2 u = s[SP(g * H + (i >> 1))];
      const float w = sl_hann((float)i * fg.inv_F);
      acc = fmaf(2.0f * ((i & 1) ? u.y : u.x), w, acc);
    }
    if constexpr (SLAB) grow[p] = acc;
    else unsafeAtomicAdd(&grow[n], acc);
  }
}

// ---- what spectral_loss.hip (the host side: sizes, workspaces, the entry points) asks of spectral_loss_det.hip ---------------
struct SlSlabFirst { long long at[16]; };              // first float of each scale's slabs, in the order of SlMulti (descending size)
// the gather's view of the slabs, scale after scale in the CALLER's order (sl_grad_gather_kernel states the contract)
struct SlGather {
  int n;
  long long first[16];                               // first float of the scale's slabs
  int nbx[16], stretch[16], step[16], pad[16];
  FastDiv step_div[16];
};
constexpr int kSlGatherThreads = 256;
void sl_launch_l1_bwd_slab(unsigned grid, hipStream_t st, const float* target, const float* audio, const float* grad_loss,
                            float* slab, int N, const SlMulti& m, float safe_eps, double* partial, const SlSlabFirst& first);
void sl_launch_l1_big_bwd_slab(dim3 grid, hipStream_t st, const float* target, const float* audio, const float* grad_loss, float* slab,
                               double* partial, int N, int n_frames, int F, float safe_eps, float mag_scale, float log_scale);
// false: no instance for a transform of S points
bool sl_launch_cot_bwd_slab(int S, dim3 grid, hipStream_t st, const float* audio, float* slab, int N, int n_frames, const float* cot);
bool sl_launch_tq_cot_bwd_slab(int S, dim3 grid, hipStream_t st, const float* audio, float* slab, int N, int n_frames,
                               const float* cot, SlFrameGeom fg);
void sl_launch_gather(const float* slab, float* grad_audio, int B, int N, const SlGather& p, bool accum, hipStream_t st);

}  // namespace ddsp
