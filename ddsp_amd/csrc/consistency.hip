// The sinusoidal consistency losses (ddsp/losses.py:689-1061: KDEConsistencyLoss, TWMLoss) and core.sinusoidal_to_harmonic
// (ddsp/core.py:733-781) for gfx950, forward and backward.
//
// The reference materialises [B, T, C, K, G], [B, T, C, P, K], [B, T, K, K] and [B, T, H, K] tensors.  Per frame the inputs are
// a few hundred floats and every output is a log-sum-exp or a weighted sum over a list that fits in LDS, so nothing of those
// sizes exists here: a block of 256 threads owns one frame, stages the frame's sinusoids once (Hz, amplitude, MIDI value and
// log2 of the normalised weight: every hz_to_midi is taken once per frame and value), and walks tiles of kTile points.
//
// One primitive.  A Gaussian mixture with centres mu_j, weights w_j (sum 1) and scale s, evaluated at a point x:
//     log p(x) = log sum_j w_j N(x; mu_j, s) = ln 2 * lse2(x) - ln s - ln(2 pi) / 2,
//     lse2(x)  = m + log2 sum_j 2^(t_j - m),   t_j = log2 w_j - c2 (x - mu_j)^2,   c2 = log2(e) / (2 s^2),   m = max_j t_j
// (max-subtracted as tfp's MixtureSameFamily.log_prob is, in base 2: v_exp_f32 / v_log_f32 are base-2 instructions).
// mix_eval walks centres staged in LDS (all lanes read the same centre: a broadcast); grid_eval is the same for the centres
// 1 .. G with uniform weights, where the maximum is at the nearest centre and needs no pass of its own.  Both also return
// dmean = sum_j p_j (x - mu_j), p_j = 2^(t_j - lse2), from which every derivative follows:
//     d(-log p)/dx = dmean / s^2,   d(-log p)/dmu_j = -p_j (x - mu_j) / s^2,   d(-log p)/d ln w_j = -p_j.
// ALL terms are summed: no Gaussian is skipped (the issue allows skipping only behind a derived rule; none is used).
//
//   twm_kernel<BWD>    TWMLoss.get_loss_tensors: p(sinusoids | harmonics) on the ratios freq_k / f0_c (C K points, the grid),
//                      p(harmonics | sinusoids) on hz_to_midi(fl32(f0_c n)) (C P points, the staged sinusoids).
//   kde_kernel<BWD>    KDEConsistencyLoss.nll: the source sinusoids as points, the target's as centres.
//   s2h_kernel<BWD>    sinusoidal_to_harmonic: exp(-(r / width)^2) on r = (freq_k - f0 h) / f0: a plain weighted sum.
//   softmin / nanargmin / mean / row_mean kernels: the reductions to the scalar (fixed-order fp64 partials).
//
// Backward: recompute, do not store.  A tile's points are evaluated once (lse2, dmean, the point's upstream coefficient, kept
// in LDS); then thread k walks the tile's points for the sums its own sinusoid owns (dL/dmu_k, dL/d ln w_k), and a wavefront
// per candidate sums the candidate's points in a fixed lane order and butterfly.  Every gradient element is written by one
// thread after sums in a fixed order: no atomics, the same bits on every run and for any sub-batch (a block sees one frame).
//
// Guards restated from the reference, op for op: safe_divide's eps 1e-7 (a denominator == 0 becomes 1e-7 and passes no
// gradient), amps == 0 -> 1e-7 (no gradient), hz_to_midi(f <= 0) = 0 (no gradient), safe_divide(mask, mean(mask)) = 0 for
// a candidate whose harmonics are all at or above Nyquist, tfd.Categorical normalising its probabilities once more
// (log w_j = log an_j - log sum an).  The Nyquist decision of TWM is taken on the MIDI values, as the reference takes it:
// equal Hz give equal MIDI and are masked; within a few ulp of Nyquist the outcome is that of log2f here and of TF's log
// there.
//
// Bounds (beyond them DDSP_ERR_UNSUPPORTED): K (and the target's K of the KDE) and H <= 1024 (staged whole in LDS),
// P <= 256, G <= 4096, any C.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "common.h"
#include "consistency_common.h"
#include "launch.h"

namespace ddsp {
namespace consistency {

constexpr int kMaxK = 1024;                 // sinusoids (centres) staged per frame
constexpr int kOwn = kMaxK / kThreads;      // sinusoids a thread owns in a backward pass: k = tid + 256 q
constexpr int kMaxH = 1024;
constexpr int kMaxP = 256;
constexpr int kMaxG = 4096;
constexpr int kTile = 2048;                 // points per tile
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kEps = 1e-7f;

static_assert(kTile >= 2 * kMaxK && kTile >= kMaxP, "a tile holds at least one candidate's points");

__device__ __forceinline__ float safe_den(float d) { return d == 0.0f ? kEps : d; }

// (kThreads, kWaves, kMidiSlope, hz_to_midi as an fp32 pair and block_sum: consistency_common.h, shared with wasserstein.hip)
__device__ __forceinline__ double wave_total(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct Centre { float mu, ml, lw2; };            // MIDI value (hi, lo), log2 of the weight

// lse2 and dmean of the mixture staged in `cen` at x
__device__ __forceinline__ void mix_eval(const Centre* cen, int J, float c2, float x, float xl, float& lse2, float& dmean) {
  float m = -INFINITY;
  for (int j = 0; j < J; ++j) {
    const Centre c = cen[j];
    const float d = (x - c.mu) + (xl - c.ml);
    m = fmaxf(m, fmaf(-c2 * d, d, c.lw2));
  }
  float S = 0.0f, dS = 0.0f;
  for (int j = 0; j < J; ++j) {
    const Centre c = cen[j];
    const float d = (x - c.mu) + (xl - c.ml);
    const float e = __builtin_amdgcn_exp2f(fmaf(-c2 * d, d, c.lw2) - m);
    S += e;
    dS = fmaf(e, d, dS);
  }
  lse2 = m + __builtin_amdgcn_logf(S);
  dmean = dS / S;
}

// the same for centres 1 .. G with weights 1 / G: the largest term is the nearest centre's
__device__ __forceinline__ void grid_eval(int G, float c2, float x, float& lse2, float& dmean) {
  const float g0 = fminf(fmaxf(rintf(x), 1.0f), (float)G);
  const float d0 = x - g0;
  const float m = c2 * d0 * d0;                       // minus the largest exponent
  float S = 0.0f, dS = 0.0f;
  for (int g = 1; g <= G; ++g) {
    const float d = x - (float)g;
    const float e = __builtin_amdgcn_exp2f(fmaf(-c2 * d, d, m));
    S += e;
    dS = fmaf(e, d, dS);
  }
  lse2 = __builtin_amdgcn_logf(S) - m - __builtin_amdgcn_logf((float)G);
  dmean = dS / S;
}

// Stages a frame's sinusoids as mixture centres: cen[k] = {hz_to_midi(freq_k), log2 w_k}, w = an / sum(an), an = a' / safe(sum a'),
// a' = where(a == 0, 1e-7, a).  Returns safe(sum a').  fr / am (may be null) receive the raw values.
__device__ __forceinline__ float stage_centres(const float* __restrict__ freqs, const float* __restrict__ amps, int K, Centre* cen,
                                               float* fr, float* am, double* red) {
  double part = 0.0;
  for (int k = threadIdx.x; k < K; k += kThreads) {
    const float f = freqs[k], a = amps[k];
    if (fr) fr[k] = f;
    if (am) am[k] = a;
    const float ap = (a == 0.0f) ? kEps : a;
    cen[k].mu = hz_to_midi(f, cen[k].ml);
    cen[k].lw2 = ap;
    part += (double)ap;
  }
  const float Dp = safe_den((float)block_sum(part, red));
  part = 0.0;
  for (int k = threadIdx.x; k < K; k += kThreads) {
    const float an = cen[k].lw2 / Dp;
    cen[k].lw2 = an;
    part += (double)an;
  }
  const float l2tot = log2f((float)block_sum(part, red));
  for (int k = threadIdx.x; k < K; k += kThreads) cen[k].lw2 = log2f(cen[k].lw2) - l2tot;
  __syncthreads();
  return Dp;
}

struct Pt { float x, xl, lse2, cg; };            // a point: its value (hi, lo), lse2 there, its upstream coefficient (or mask)

// ---- TWMLoss.get_loss_tensors ------------------------------------------------------------------------------------------------
struct TwmArgs {
  int C, K, P, G;
  float c2_s, inv_s2_s, cst_s;          // p(sinusoids | harmonics): harmonics_scale; nll = -(ln2 lse2 + cst)
  float c2_h, inv_s2_h, cst_h;          // p(harmonics | sinusoids): sinusoids_scale
  float nyquist;
};

__device__ __forceinline__ float harmonic_prior(int n, int P) {      // tf.linspace(1, 1 / P, P)[n]
  return P > 1 ? (float)(1.0 + (double)n * ((1.0 / (double)P - 1.0) / (double)(P - 1))) : 1.0f;
}

template <bool BWD>
__global__ __launch_bounds__(kThreads) void twm_kernel(const float* __restrict__ f0c /*[R,C]*/, const float* __restrict__ freqs /*[R,K]*/,
                                                       const float* __restrict__ amps /*[R,K]*/, float* __restrict__ sin_loss /*[R,C]*/,
                                                       float* __restrict__ harm_loss /*[R,C]*/, const float* __restrict__ g_sin,
                                                       const float* __restrict__ g_harm, float* __restrict__ g_f0c,
                                                       float* __restrict__ g_freqs, float* __restrict__ g_amps, TwmArgs p) {
  __shared__ Centre s_cen[kMaxK];
  __shared__ float s_fr[kMaxK], s_am[kMaxK];
  __shared__ Pt s_pt[kTile];
  __shared__ float s_dm[kTile];                      // d nll / dx of a point
  __shared__ double s_red[kWaves];
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = p.C, K = p.K, P = p.P;
  f0c += row * C; freqs += row * K; amps += row * K;
  sin_loss += row * C;
  if (!BWD) harm_loss += row * C;
  if (BWD) { g_sin += row * C; g_harm += row * C; g_f0c += row * C; g_freqs += row * K; g_amps += row * K; }

  const float Dp = stage_centres(freqs, amps, K, s_cen, s_fr, s_am, s_red);
  double part = 0.0;
  for (int k = tid; k < K; k += kThreads) part += (double)s_am[k];
  const float sumA = (float)block_sum(part, s_red);
  const float D = safe_den(sumA);
  const float nyq_midi = hz_to_midi(p.nyquist);

  float acc_fr[kOwn], acc_am[kOwn], acc_q[kOwn], acc_r[kOwn];
#pragma unroll
  for (int q = 0; q < kOwn; ++q) acc_fr[q] = acc_am[q] = acc_q[q] = acc_r[q] = 0.0f;

  // ---- p(sinusoids | harmonics): points (c, k), x = safe_divide(freq_k, f0_c) ------------------------------------------------
  const int ct_s = kTile / K;
  for (int c0 = 0; c0 < C; c0 += ct_s) {
    const int nc = min(ct_s, C - c0), npts = nc * K;
    for (int i = tid; i < npts; i += kThreads) {
      const int cl = i / K, k = i - cl * K;
      const float x = s_fr[k] / safe_den(f0c[c0 + cl]);
      float lse2, dmean;
      grid_eval(p.G, p.c2_s, x, lse2, dmean);
      Pt pt;
      pt.x = -(kLn2 * lse2 + p.cst_s);              // nll
      pt.xl = 0.0f; pt.lse2 = 0.0f; pt.cg = 0.0f;
      s_pt[i] = pt;
      s_dm[i] = dmean * p.inv_s2_s;                 // d nll / dx
    }
    __syncthreads();
    for (int cl = wave; cl < nc; cl += kWaves) {
      const Pt* pts = s_pt + cl * K;
      double s = 0.0, v = 0.0;
      for (int k = lane; k < K; k += 64) {
        s += (double)(pts[k].x * s_am[k]);
        if (BWD) v += (double)(s_am[k] * s_dm[cl * K + k] * s_fr[k]);
      }
      s = wave_total(s);
      if (BWD) v = wave_total(v);
      if (lane == 0) {
        if (!BWD) {
          sin_loss[c0 + cl] = (float)s / D;
        } else {
          const float f0 = f0c[c0 + cl];
          // x = freq_k / f0: dx / df0 = -freq_k / f0^2 (a zero f0 was replaced by a constant: no gradient)
          g_f0c[c0 + cl] = (f0 != 0.0f) ? g_sin[c0 + cl] / D * (-(float)v / (f0 * f0)) : 0.0f;
        }
      }
    }
    if (BWD) {
#pragma unroll
      for (int q = 0; q < kOwn; ++q) {
        const int k = tid + q * kThreads;
        if (k < K) {
          const float a = s_am[k];
          for (int cl = 0; cl < nc; ++cl) {
            const Pt pt = s_pt[cl * K + k];
            const float gs = g_sin[c0 + cl];
            const float S = (sumA != 0.0f) ? sin_loss[c0 + cl] : 0.0f;       // d safe(sum a) / da = 0 when the sum was replaced
            acc_am[q] += gs * (pt.x - S) / D;
            acc_fr[q] += gs * a / D * s_dm[cl * K + k] / safe_den(f0c[c0 + cl]);
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- p(harmonics | sinusoids): points (c, n), x = hz_to_midi(fl32(f0_c n)) -------------------------------------------------
  const int ct_h = kTile / P;
  for (int c0 = 0; c0 < C; c0 += ct_h) {
    const int nc = min(ct_h, C - c0), npts = nc * P;
    for (int i = tid; i < npts; i += kThreads) {
      const int cl = i / P, n = i - cl * P;
      const float hz = rn_mul(f0c[c0 + cl], (float)(n + 1));
      Pt pt;
      float dmean;
      pt.x = hz_to_midi(hz, pt.xl);
      mix_eval(s_cen, K, p.c2_h, pt.x, pt.xl, pt.lse2, dmean);
      pt.cg = (pt.x < nyq_midi) ? 1.0f : 0.0f;
      s_pt[i] = pt;
      s_dm[i] = dmean * p.inv_s2_h;                 // d nll / dx
    }
    __syncthreads();
    for (int cl = wave; cl < nc; cl += kWaves) {
      Pt* pts = s_pt + cl * P;
      double cnt = 0.0;
      for (int n = lane; n < P; n += 64) cnt += (double)pts[n].cg;
      const float mean_mask = (float)wave_total(cnt) / (float)P;
      const float sm = safe_den(mean_mask);
      double s = 0.0, v = 0.0;
      for (int n = lane; n < P; n += 64) {
        const float w = harmonic_prior(n, P) * (pts[n].cg / sm);
        if (!BWD) {
          s += (double)(-(kLn2 * pts[n].lse2 + p.cst_h) * w);
        } else {
          const float cg = g_harm[c0 + cl] * w / (float)P;          // d loss / d nll of this point
          pts[n].cg = cg;
          const float hz = rn_mul(f0c[c0 + cl], (float)(n + 1));
          // d nll / dx = dmean / s^2; dx / df0 = n kMidiSlope / hz = kMidiSlope / f0 where hz > 0
          if (hz > 0.0f) v += (double)(cg * s_dm[cl * P + n]);
        }
      }
      if (!BWD) {
        s = wave_total(s);
        if (lane == 0) harm_loss[c0 + cl] = (float)s / (float)P;
      } else {
        v = wave_total(v);
        if (lane == 0) g_f0c[c0 + cl] += (float)v * kMidiSlope / safe_den(f0c[c0 + cl]);
      }
    }
    if (BWD) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kOwn; ++q) {
        const int k = tid + q * kThreads;
        if (k < K) {
          const Centre c = s_cen[k];
          float aq = 0.0f, ar = 0.0f;
          for (int i = 0; i < npts; ++i) {
            const Pt pt = s_pt[i];
            const float d = (pt.x - c.mu) + (pt.xl - c.ml);
            const float pj = pt.cg * __builtin_amdgcn_exp2f(fmaf(-p.c2_h * d, d, c.lw2) - pt.lse2);
            aq += pj;
            ar = fmaf(pj, d, ar);
          }
          acc_q[q] += aq;
          acc_r[q] += ar;
        }
      }
    }
    __syncthreads();
  }

  if (BWD) {
    double qs = 0.0;
#pragma unroll
    for (int q = 0; q < kOwn; ++q) qs += (double)acc_q[q];
    const float Q = (float)block_sum(qs, s_red);
#pragma unroll
    for (int q = 0; q < kOwn; ++q) {
      const int k = tid + q * kThreads;
      if (k < K) {
        const float f = s_fr[k], a = s_am[k];
        // d nll / dmu_k = -p_k (x - mu_k) / s^2; dmu / dfreq = kMidiSlope / freq where freq > 0
        g_freqs[k] = acc_fr[q] + (f > 0.0f ? -acc_r[q] * p.inv_s2_h * kMidiSlope / f : 0.0f);
        // ln w_k = ln a'_k - ln sum a': d loss / da'_k = -q_k / a'_k + Q / sum a'; the replaced zeros pass nothing
        g_amps[k] = acc_am[q] + (a != 0.0f ? -acc_q[q] / a + Q / Dp : 0.0f);
      }
    }
  }
}

// ---- KDEConsistencyLoss.nll ------------------------------------------------------------------------------------------------
struct KdeArgs { int K, Kt; float c2, inv_s2, cst; };

template <bool BWD>
__global__ __launch_bounds__(kThreads) void kde_kernel(const float* __restrict__ amps /*[R,K]*/, const float* __restrict__ freqs,
                                                       const float* __restrict__ amps_t /*[R,Kt]*/, const float* __restrict__ freqs_t,
                                                       float* __restrict__ nll_out /*[R]*/, const float* __restrict__ g_nll,
                                                       float* __restrict__ g_amps, float* __restrict__ g_freqs,
                                                       float* __restrict__ g_amps_t, float* __restrict__ g_freqs_t, KdeArgs p) {
  __shared__ Centre s_cen[kMaxK];
  __shared__ float s_frt[kMaxK], s_amt[kMaxK];
  __shared__ Pt s_pt[kMaxK];
  __shared__ float s_dm[kMaxK];
  __shared__ double s_red[kWaves];
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const int K = p.K, Kt = p.Kt;
  amps += row * K; freqs += row * K; amps_t += row * Kt; freqs_t += row * Kt;
  const float Dp = stage_centres(freqs_t, amps_t, Kt, s_cen, s_frt, s_amt, s_red);

  double sa = 0.0, sn = 0.0;
  for (int k = tid; k < K; k += kThreads) {
    const float a = amps[k];
    Pt pt;
    float dmean;
    pt.x = hz_to_midi(freqs[k], pt.xl);
    mix_eval(s_cen, Kt, p.c2, pt.x, pt.xl, pt.lse2, dmean);
    pt.cg = a;
    if (BWD) { s_pt[k] = pt; s_dm[k] = dmean; }
    sa += (double)a;
    sn += (double)(-(kLn2 * pt.lse2 + p.cst) * a);
  }
  const float sumA = (float)block_sum(sa, s_red);
  const float N = (float)block_sum(sn, s_red);
  const float D = safe_den(sumA);
  if (!BWD) {
    if (tid == 0) nll_out[row] = N / D / (float)K;
    return;
  }
  const float g = g_nll[row] / (float)K;
  g_amps += row * K; g_freqs += row * K; g_amps_t += row * Kt; g_freqs_t += row * Kt;
  for (int k = tid; k < K; k += kThreads) {
    const Pt pt = s_pt[k];
    const float nll = -(kLn2 * pt.lse2 + p.cst), a = pt.cg, f = freqs[k];
    g_amps[k] = g * (nll - (sumA != 0.0f ? N / D : 0.0f)) / D;
    const float cg = g * a / D;
    g_freqs[k] = f > 0.0f ? cg * s_dm[k] * p.inv_s2 * kMidiSlope / f : 0.0f;
    s_pt[k].cg = cg;
  }
  __syncthreads();
  float acc_q[kOwn], acc_r[kOwn];
  double qs = 0.0;
#pragma unroll
  for (int q = 0; q < kOwn; ++q) {
    acc_q[q] = acc_r[q] = 0.0f;
    const int j = tid + q * kThreads;
    if (j < Kt) {
      const Centre c = s_cen[j];
      for (int i = 0; i < K; ++i) {
        const Pt pt = s_pt[i];
        const float d = (pt.x - c.mu) + (pt.xl - c.ml);
        const float pj = pt.cg * __builtin_amdgcn_exp2f(fmaf(-p.c2 * d, d, c.lw2) - pt.lse2);
        acc_q[q] += pj;
        acc_r[q] = fmaf(pj, d, acc_r[q]);
      }
    }
    qs += (double)acc_q[q];
  }
  const float Q = (float)block_sum(qs, s_red);
#pragma unroll
  for (int q = 0; q < kOwn; ++q) {
    const int j = tid + q * kThreads;
    if (j < Kt) {
      const float f = s_frt[j], a = s_amt[j];
      g_freqs_t[j] = f > 0.0f ? -acc_r[q] * p.inv_s2 * kMidiSlope / f : 0.0f;
      g_amps_t[j] = a != 0.0f ? -acc_q[q] / a + Q / Dp : 0.0f;
    }
  }
}

// ---- core.sinusoidal_to_harmonic ---------------------------------------------------------------------------------------------
struct S2hArgs { int K, H; float inv_w2, nyquist; int normalize; };

template <bool BWD>
__global__ __launch_bounds__(kThreads) void s2h_kernel(const float* __restrict__ sin_amps /*[R,K]*/, const float* __restrict__ sin_freqs,
                                                       const float* __restrict__ f0_hz /*[R]*/, float* __restrict__ harm_amp /*[R]*/,
                                                       float* __restrict__ harm_dist /*[R,H]*/, const float* __restrict__ g_amp,
                                                       const float* __restrict__ g_dist, float* __restrict__ g_sin_amps,
                                                       float* __restrict__ g_sin_freqs, float* __restrict__ g_f0, S2hArgs p) {
  __shared__ float s_fr[kMaxK], s_am[kMaxK];
  __shared__ float s_ha[kMaxH], s_gw[kMaxH], s_shift[kMaxH];
  __shared__ double s_red[kWaves];
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const int K = p.K, H = p.H;
  sin_amps += row * K; sin_freqs += row * K;
  if (!BWD) harm_dist += row * H;
  for (int k = tid; k < K; k += kThreads) { s_fr[k] = sin_freqs[k]; s_am[k] = sin_amps[k]; }
  __syncthreads();
  const float f0 = f0_hz[row], sf0 = safe_den(f0);

  double part = 0.0;
  for (int h = tid; h < H; h += kThreads) {
    const float hf = rn_mul(f0, (float)(h + 1));
    float W = 0.0f, U = 0.0f;
    for (int k = 0; k < K; ++k) {
      const float r = (s_fr[k] - hf) / sf0;                            // (the product rounded first, as the reference's)
      const float w = __builtin_amdgcn_exp2f(-kLog2e * p.inv_w2 * r * r);
      W += w;
      U = fmaf(w, s_am[k], U);
    }
    const bool norm = p.normalize && W > 1.0f;
    float ha = norm ? U / W : U;
    const bool masked = hf >= p.nyquist;
    if (masked) ha = 0.0f;
    s_ha[h] = ha;
    if (BWD) {
      s_gw[h] = masked ? 0.0f : (norm ? 1.0f / W : 1.0f);
      s_shift[h] = norm ? U / W : 0.0f;
    }
    part += (double)ha;
  }
  const float A = (float)block_sum(part, s_red);
  const float SA = safe_den(A);
  if (!BWD) {
    if (tid == 0) harm_amp[row] = A;
    for (int h = tid; h < H; h += kThreads) harm_dist[h] = s_ha[h] / SA;
    return;
  }
  g_dist += row * H; g_sin_amps += row * K; g_sin_freqs += row * K;
  part = 0.0;
  for (int h = tid; h < H; h += kThreads) part += (double)(g_dist[h] * s_ha[h]);
  const float Bsum = (float)block_sum(part, s_red);
  const float Bs = (A != 0.0f) ? Bsum / (SA * SA) : 0.0f;            // (a zero sum was replaced by a constant: no gradient through it)
  const float ga = g_amp[row];
  // dist_h = ha_h / safe(A): d loss / d ha_h = g_amp + g_dist_h / SA - sum(g_dist ha) / SA^2
  for (int h = tid; h < H; h += kThreads) s_gw[h] *= ga + g_dist[h] / SA - Bs;
  __syncthreads();
  double pf0 = 0.0;
  for (int k = tid; k < K; k += kThreads) {
    const float fr = s_fr[k], a = s_am[k];
    float gak = 0.0f, gfk = 0.0f, gf0 = 0.0f;
    for (int h = 0; h < H; ++h) {
      const float n = (float)(h + 1);
      const float r = (fr - rn_mul(f0, n)) / sf0;
      const float w = __builtin_amdgcn_exp2f(-kLog2e * p.inv_w2 * r * r);
      const float gw = s_gw[h];
      gak = fmaf(gw, w, gak);
      // ha_h = sum_k w a (/ W): d ha / dw_hk = (a_k - shift_h) gw; dw / dr = -2 r w / width^2
      const float t = gw * (a - s_shift[h]) * w * (-2.0f * r * p.inv_w2);
      gfk += t / sf0;
      gf0 += t * (-n / sf0 - (f0 != 0.0f ? r / sf0 : 0.0f));
    }
    g_sin_amps[k] = gak;
    g_sin_freqs[k] = gfk;
    pf0 += (double)gf0;
  }
  const float tot = (float)block_sum(pf0, s_red);
  if (tid == 0) g_f0[row] = tot;
}

// ---- the reductions to the scalar --------------------------------------------------------------------------------------------
// TWMLoss.call per frame: L_c = w_s S_c + w_h H_c, out = sum_c L_c softmax(-L / temperature)_c.  BWD: g [R] -> g_S, g_H [R,C],
// d out / dL_c = p_c (1 - (L_c - out) / temperature).  A thread per frame, the candidates in index order.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void softmin_kernel(const float* __restrict__ S, const float* __restrict__ Hl, float* __restrict__ out,
                                                           const float* __restrict__ g, float* __restrict__ gS, float* __restrict__ gH,
                                                           size_t rows, int C, float ws, float wh, float inv_temp) {
  const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= rows) return;
  const float* s = S + r * C;
  const float* h = Hl + r * C;
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmaxf(m, -(ws * s[c] + wh * h[c]) * inv_temp);
  float Z = 0.0f, E = 0.0f;
  for (int c = 0; c < C; ++c) {
    const float L = ws * s[c] + wh * h[c];
    const float e = expf(-L * inv_temp - m);
    Z += e;
    E = fmaf(L, e, E);
  }
  E /= Z;
  if (!BWD) { out[r] = E; return; }
  const float gr = g[r];
  for (int c = 0; c < C; ++c) {
    const float L = ws * s[c] + wh * h[c];
    const float pc = expf(-L * inv_temp - m) / Z;
    const float d = gr * pc * (1.0f - (L - E) * inv_temp);
    gS[r * C + c] = ws * d;
    gH[r * C + c] = wh * d;
  }
}

// TWMLoss.predict_f0: np.nanargmin over the candidates (the first of equal minima), the candidate gathered; a frame of NaNs
// alone raises the flag.
__global__ __launch_bounds__(kThreads) void nanargmin_kernel(const float* __restrict__ S, const float* __restrict__ Hl,
                                                             const float* __restrict__ f0c, float* __restrict__ out, int* __restrict__ flag,
                                                             size_t rows, int C, float ws, float wh) {
  const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= rows) return;
  int best = -1;
  float bl = 0.0f;
  for (int c = 0; c < C; ++c) {
    const float L = ws * S[r * C + c] + wh * Hl[r * C + c];
    if (L != L) continue;
    if (best < 0 || L < bl) { best = c; bl = L; }
  }
  if (best < 0) { *flag = 1; best = 0; }              // (every writer stores the same value: plain vector stores)
  out[r] = f0c[r * C + best];
}

// out = scale * sum(x) / n: one block, lane-strided fp64 partials in a fixed order
__global__ __launch_bounds__(kThreads) void mean_kernel(const float* __restrict__ x, size_t n, double scale, float* __restrict__ out) {
  __shared__ double s_red[kWaves];
  double part = 0.0;
  for (size_t i = threadIdx.x; i < n; i += kThreads) part += (double)x[i];
  const double tot = block_sum(part, s_red);
  if (threadIdx.x == 0) out[0] = (float)(scale * tot / (double)n);
}
// its adjoint: out[i] = coef * g[0]
__global__ __launch_bounds__(kThreads) void fill_scaled_kernel(const float* __restrict__ g, float coef, float* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) out[i] = coef * g[0];
}
// tf.reduce_mean(x, axis=-1) and its adjoint
template <bool BWD>
__global__ __launch_bounds__(kThreads) void row_mean_kernel(const float* __restrict__ in, float* __restrict__ out, size_t rows, int K) {
  const size_t r = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (!BWD) {
    if (r >= rows) return;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += (double)in[r * K + k];
    out[r] = (float)(s / (double)K);
  } else {
    if (r >= rows * (size_t)K) return;
    out[r] = in[r / K] / (float)K;
  }
}
// adjoints of the conversions the losses differentiate through: hz_to_midi and log10(max(amin, x))
__global__ __launch_bounds__(kThreads) void convert_backward_kernel(const float* __restrict__ in, const float* __restrict__ g,
                                                                    float* __restrict__ out, size_t n, int op, float p0, float p1) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float x = in[i];
  float d;
  if (op == DDSP_CONVERT_HZ_TO_MIDI) d = x > 0.0f ? kMidiSlope / x : 0.0f;
  else d = (x > p1 && x > 0.0f) ? 1.0f / (x * p0) : 0.0f;      // LOG_FLOOR: tf.maximum(amin, x) passes the gradient to x where x > amin
  out[i] = g[i] * d;
}

static unsigned blocks_for(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }
static bool rows_ok(size_t rows) { return rows > 0 && rows <= (size_t)0x7fffffff; }

static int make_twm(TwmArgs* a, int C, int K, int P, int G, float sinusoids_scale, float harmonics_scale, float sample_rate) {
  if (C <= 0 || K <= 0 || P <= 0 || G <= 0 || !(sinusoids_scale > 0.0f) || !(harmonics_scale > 0.0f) || !(sample_rate > 0.0f))
    return DDSP_ERR_BAD_SHAPE;
  if (K > kMaxK || P > kMaxP || G > kMaxG) return DDSP_ERR_UNSUPPORTED;
  a->C = C; a->K = K; a->P = P; a->G = G;
  const double hs = harmonics_scale, ss = sinusoids_scale;
  a->c2_s = (float)(0.5 * 1.4426950408889634 / (hs * hs)); a->inv_s2_s = (float)(1.0 / (hs * hs));
  a->cst_s = (float)(-log(hs) - 0.9189385332046727);
  a->c2_h = (float)(0.5 * 1.4426950408889634 / (ss * ss)); a->inv_s2_h = (float)(1.0 / (ss * ss));
  a->cst_h = (float)(-log(ss) - 0.9189385332046727);
  a->nyquist = sample_rate / 2.0f;
  return DDSP_OK;
}

}  // namespace consistency
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::consistency;

extern "C" int ddsp_twm_loss_tensors_f32(const float* f0_candidates, const float* freqs, const float* amps, float* sinusoids_loss,
                                         float* harmonics_loss, size_t rows, int C, int K, int n_harmonic_points,
                                         int n_harmonic_gaussians, float sinusoids_scale, float harmonics_scale, float sample_rate,
                                         void* stream) {
  if (!f0_candidates || !freqs || !amps || !sinusoids_loss || !harmonics_loss) return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows)) return DDSP_ERR_BAD_SHAPE;
  TwmArgs a;
  const int rc = make_twm(&a, C, K, n_harmonic_points, n_harmonic_gaussians, sinusoids_scale, harmonics_scale, sample_rate);
  if (rc != DDSP_OK) return rc;
  hipLaunchKernelGGL((twm_kernel<false>), dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, f0_candidates, freqs, amps,
                     sinusoids_loss, harmonics_loss, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr, a);
  return check_launch();
}

extern "C" int ddsp_twm_loss_tensors_backward_f32(const float* f0_candidates, const float* freqs, const float* amps,
                                                  const float* sinusoids_loss, const float* grad_sinusoids_loss,
                                                  const float* grad_harmonics_loss, float* grad_f0_candidates, float* grad_freqs,
                                                  float* grad_amps, size_t rows, int C, int K, int n_harmonic_points,
                                                  int n_harmonic_gaussians, float sinusoids_scale, float harmonics_scale,
                                                  float sample_rate, void* stream) {
  if (!f0_candidates || !freqs || !amps || !sinusoids_loss || !grad_sinusoids_loss || !grad_harmonics_loss || !grad_f0_candidates ||
      !grad_freqs || !grad_amps)
    return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows)) return DDSP_ERR_BAD_SHAPE;
  TwmArgs a;
  const int rc = make_twm(&a, C, K, n_harmonic_points, n_harmonic_gaussians, sinusoids_scale, harmonics_scale, sample_rate);
  if (rc != DDSP_OK) return rc;
  hipLaunchKernelGGL((twm_kernel<true>), dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, f0_candidates, freqs, amps,
                     const_cast<float*>(sinusoids_loss), (float*)nullptr, grad_sinusoids_loss, grad_harmonics_loss, grad_f0_candidates,
                     grad_freqs, grad_amps, a);
  return check_launch();
}

static int make_kde(KdeArgs* a, int K, int Kt, float scale) {
  if (K <= 0 || Kt <= 0 || !(scale > 0.0f)) return DDSP_ERR_BAD_SHAPE;
  if (K > kMaxK || Kt > kMaxK) return DDSP_ERR_UNSUPPORTED;
  const double s = scale;
  a->K = K; a->Kt = Kt;
  a->c2 = (float)(0.5 * 1.4426950408889634 / (s * s)); a->inv_s2 = (float)(1.0 / (s * s));
  a->cst = (float)(-log(s) - 0.9189385332046727);
  return DDSP_OK;
}

extern "C" int ddsp_kde_nll_f32(const float* amps, const float* freqs, const float* amps_target, const float* freqs_target, float* nll,
                                size_t rows, int K, int K_target, float scale_target, void* stream) {
  if (!amps || !freqs || !amps_target || !freqs_target || !nll) return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows)) return DDSP_ERR_BAD_SHAPE;
  KdeArgs a;
  const int rc = make_kde(&a, K, K_target, scale_target);
  if (rc != DDSP_OK) return rc;
  hipLaunchKernelGGL((kde_kernel<false>), dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, amps, freqs, amps_target,
                     freqs_target, nll, (const float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, a);
  return check_launch();
}

extern "C" int ddsp_kde_nll_backward_f32(const float* amps, const float* freqs, const float* amps_target, const float* freqs_target,
                                         const float* grad_nll, float* grad_amps, float* grad_freqs, float* grad_amps_target,
                                         float* grad_freqs_target, size_t rows, int K, int K_target, float scale_target, void* stream) {
  if (!amps || !freqs || !amps_target || !freqs_target || !grad_nll || !grad_amps || !grad_freqs || !grad_amps_target ||
      !grad_freqs_target)
    return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows)) return DDSP_ERR_BAD_SHAPE;
  KdeArgs a;
  const int rc = make_kde(&a, K, K_target, scale_target);
  if (rc != DDSP_OK) return rc;
  hipLaunchKernelGGL((kde_kernel<true>), dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, amps, freqs, amps_target,
                     freqs_target, (float*)nullptr, grad_nll, grad_amps, grad_freqs, grad_amps_target, grad_freqs_target, a);
  return check_launch();
}

static int make_s2h(S2hArgs* a, int K, int H, float harmonic_width, float sample_rate, unsigned flags) {
  if (K <= 0 || H <= 0 || !(sample_rate > 0.0f) || harmonic_width == 0.0f) return DDSP_ERR_BAD_SHAPE;
  if (K > kMaxK || H > kMaxH) return DDSP_ERR_UNSUPPORTED;
  a->K = K; a->H = H;
  a->inv_w2 = (float)(1.0 / ((double)harmonic_width * (double)harmonic_width));
  a->nyquist = sample_rate / 2.0f;
  a->normalize = (flags & DDSP_S2H_NORMALIZE) ? 1 : 0;
  return DDSP_OK;
}

extern "C" int ddsp_sinusoidal_to_harmonic_f32(const float* sin_amps, const float* sin_freqs, const float* f0_hz, float* harm_amp,
                                               float* harm_dist, size_t rows, int K, int H, float harmonic_width, float sample_rate,
                                               unsigned flags, void* stream) {
  if (!sin_amps || !sin_freqs || !f0_hz || !harm_amp || !harm_dist) return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows)) return DDSP_ERR_BAD_SHAPE;
  S2hArgs a;
  const int rc = make_s2h(&a, K, H, harmonic_width, sample_rate, flags);
  if (rc != DDSP_OK) return rc;
  hipLaunchKernelGGL((s2h_kernel<false>), dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, sin_amps, sin_freqs, f0_hz,
                     harm_amp, harm_dist, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr, a);
  return check_launch();
}

extern "C" int ddsp_sinusoidal_to_harmonic_backward_f32(const float* sin_amps, const float* sin_freqs, const float* f0_hz,
                                                        const float* grad_harm_amp, const float* grad_harm_dist, float* grad_sin_amps,
                                                        float* grad_sin_freqs, float* grad_f0_hz, size_t rows, int K, int H,
                                                        float harmonic_width, float sample_rate, unsigned flags, void* stream) {
  if (!sin_amps || !sin_freqs || !f0_hz || !grad_harm_amp || !grad_harm_dist || !grad_sin_amps || !grad_sin_freqs || !grad_f0_hz)
    return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows)) return DDSP_ERR_BAD_SHAPE;
  S2hArgs a;
  const int rc = make_s2h(&a, K, H, harmonic_width, sample_rate, flags);
  if (rc != DDSP_OK) return rc;
  hipLaunchKernelGGL((s2h_kernel<true>), dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, sin_amps, sin_freqs, f0_hz,
                     (float*)nullptr, (float*)nullptr, grad_harm_amp, grad_harm_dist, grad_sin_amps, grad_sin_freqs,
                     grad_f0_hz, a);
  return check_launch();
}

extern "C" int ddsp_twm_softmin_f32(const float* sinusoids_loss, const float* harmonics_loss, float* frame_loss, size_t rows, int C,
                                    float sinusoids_weight, float harmonics_weight, float temperature, void* stream) {
  if (!sinusoids_loss || !harmonics_loss || !frame_loss) return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows) || C <= 0 || !(temperature > 0.0f)) return DDSP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL((softmin_kernel<false>), dim3(blocks_for(rows)), dim3(kThreads), 0, (hipStream_t)stream, sinusoids_loss,
                     harmonics_loss, frame_loss, (const float*)nullptr, (float*)nullptr, (float*)nullptr, rows, C, sinusoids_weight,
                     harmonics_weight, 1.0f / temperature);
  return check_launch();
}

extern "C" int ddsp_twm_softmin_backward_f32(const float* sinusoids_loss, const float* harmonics_loss, const float* grad_frame_loss,
                                             float* grad_sinusoids_loss, float* grad_harmonics_loss, size_t rows, int C,
                                             float sinusoids_weight, float harmonics_weight, float temperature, void* stream) {
  if (!sinusoids_loss || !harmonics_loss || !grad_frame_loss || !grad_sinusoids_loss || !grad_harmonics_loss) return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows) || C <= 0 || !(temperature > 0.0f)) return DDSP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL((softmin_kernel<true>), dim3(blocks_for(rows)), dim3(kThreads), 0, (hipStream_t)stream, sinusoids_loss,
                     harmonics_loss, (float*)nullptr, grad_frame_loss, grad_sinusoids_loss, grad_harmonics_loss, rows, C,
                     sinusoids_weight, harmonics_weight, 1.0f / temperature);
  return check_launch();
}

extern "C" int ddsp_twm_nanargmin_f32(const float* sinusoids_loss, const float* harmonics_loss, const float* f0_candidates, float* f0_hz,
                                      int* all_nan_flag, size_t rows, int C, float sinusoids_weight, float harmonics_weight,
                                      void* stream) {
  if (!sinusoids_loss || !harmonics_loss || !f0_candidates || !f0_hz || !all_nan_flag) return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows) || C <= 0) return DDSP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(nanargmin_kernel, dim3(blocks_for(rows)), dim3(kThreads), 0, (hipStream_t)stream, sinusoids_loss, harmonics_loss,
                     f0_candidates, f0_hz, all_nan_flag, rows, C, sinusoids_weight, harmonics_weight);
  return check_launch();
}

extern "C" int ddsp_mean_f32(const float* x, float* out, size_t n, float scale, void* stream) {
  if (!x || !out) return DDSP_ERR_NULL_POINTER;
  if (n == 0) return DDSP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, x, n, (double)scale, out);
  return check_launch();
}

extern "C" int ddsp_mean_backward_f32(const float* grad_out, float* grad_x, size_t n, float scale, void* stream) {
  if (!grad_out || !grad_x) return DDSP_ERR_NULL_POINTER;
  if (n == 0 || n > (size_t)0x7fffffff * kThreads) return DDSP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(fill_scaled_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, grad_out,
                     (float)((double)scale / (double)n), grad_x, n);
  return check_launch();
}

extern "C" int ddsp_row_mean_f32(const float* x, float* out, size_t rows, int K, void* stream) {
  if (!x || !out) return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows) || K <= 0) return DDSP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL((row_mean_kernel<false>), dim3(blocks_for(rows)), dim3(kThreads), 0, (hipStream_t)stream, x, out, rows, K);
  return check_launch();
}

extern "C" int ddsp_row_mean_backward_f32(const float* grad_out, float* grad_x, size_t rows, int K, void* stream) {
  if (!grad_out || !grad_x) return DDSP_ERR_NULL_POINTER;
  if (!rows_ok(rows) || K <= 0) return DDSP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL((row_mean_kernel<true>), dim3(blocks_for(rows * (size_t)K)), dim3(kThreads), 0, (hipStream_t)stream, grad_out,
                     grad_x, rows, K);
  return check_launch();
}

extern "C" int ddsp_unit_convert_backward_f32(const float* in, const float* grad_out, float* grad_in, size_t n, int op, float p0,
                                              float p1, void* stream) {
  if (!in || !grad_out || !grad_in) return DDSP_ERR_NULL_POINTER;
  if (n == 0 || n > (size_t)0x7fffffff * kThreads) return DDSP_ERR_BAD_SHAPE;
  if (op != DDSP_CONVERT_HZ_TO_MIDI && op != DDSP_CONVERT_LOG_FLOOR) return DDSP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(convert_backward_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, in, grad_out, grad_in, n, op,
                     p0, p1);
  return check_launch();
}
