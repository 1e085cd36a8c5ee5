// synths.Sinusoidal (ddsp/synths.py:260-323) for gfx950, forward and backward, with the frequency scale functions under it
// (core.frequencies_sigmoid / frequencies_softmax and the unit / MIDI / Hz conversions, ddsp/core.py:219-348, 414-507).
//
// The reference resamples amplitudes and frequencies to audio rate ([B, N, K] each) and hands both to oscillator_bank, which
// reads the frequency envelope twice.  Everything a sample needs is a function of the controls of its frame and the next
// one, so nothing of that size exists here:
//
//   sin_controls_kernel   frame rate: exp_sigmoid on the amplitudes, the frequency scale function (depth and Hz range are
//                         arguments; the MIDI constants of frequencies_sigmoid's `depth` terms are made on the host),
//                         remove_above_nyquist.  <BWD> is its adjoint.
//   sin_prefix_kernel     frame rate: per (row, sinusoid) the phase at the start of every frame, in cycles, summed in fp64
//                         (16 segments of frames per sinusoid, a prefix over the segments, then the running sum) and stored
//                         wrapped to [0, 1) as fp32 (2^-25 cycles).
//   sin_synth_kernel      a block per (row, 1024 samples), a thread per sample (four of them, 256 apart): the coefficient
//                         sets of the frames the run touches are staged in LDS per tile of sinusoids, then every thread
//                         walks the sinusoids in index order (a fixed order of additions).
//   sin_bwd_sums_kernel   a thread per (row, frame, sinusoid) walks the frame's samples and leaves five sums; no reduction
//   sin_bwd_scan_kernel   across threads and no atomics anywhere.  The scan takes the suffix over the frames in fp64 and
//                         assembles dL/d amplitudes and dL/d frequencies at frame rate.
//
// Phase.  The frequency envelope is TF's legacy bilinear resize, f_j + (f_{j+1} - f_j) r / hop inside frame j (the last frame
// held), and tf.cumsum is INCLUSIVE, so with c0 the cycles before the frame, c1 = f_j / sr and c2 = (f_{j+1} - f_j) / (hop sr)
//     phase(r) = c0 + (r + 1) c1 + (r (r + 1) / 2) c2        [cycles]
// A frame of 2048 samples holds up to 1024 cycles and the quadratic term needs 45 bits for 2^-22 cycles, so the three terms
// are two fp64 FMAs, wrapped by v_fract_f64 BEFORE the conversion to fp32 (the vector ALU issues fp64 FMAs at the fp32 rate).
// v_sin_f32 / v_cos_f32 take cycles.
//
// oscillator_bank masks at audio rate: a sample whose interpolated frequency is >= sr / 2 contributes nothing (and passes no
// gradient).  The fp32 interpolation is monotone, so only frames with ONE endpoint at or above Nyquist need the per-sample
// test; a block that stages such a frame runs the loop instance with the test, every other block the one without.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "profile.h"
#include "launch.h"
#include "nan_select.h"

namespace ddsp {
namespace sinusoidal {

constexpr int kThreads = 256;
constexpr int kSamplesPerThread = 4;
constexpr int kChunk = kThreads * kSamplesPerThread;   // samples per block of sin_synth_kernel
constexpr int kMaxEntries = 1280;                      // (frame, sinusoid) coefficient sets in LDS: 50 KB, three blocks per CU
constexpr int kMaxDepth = 64;                          // terms of frequencies_sigmoid whose constants travel as kernel arguments
constexpr int kSegs = 16, kLanesK = 16;                // frame-rate scans: 16 sinusoids x 16 segments of frames per block
constexpr int kRChunk = 1024;                          // sin_bwd_sums_kernel: window weights tabulated per run of samples
constexpr float kLn10 = 2.302585092994046f;
constexpr float kLn2Over12 = 0.057762265046662105f;

static_assert(kLanesK * kSegs == kThreads, "one thread per (sinusoid, segment)");
static_assert(kChunk + 1 <= kMaxEntries, "a run of kChunk frames of one sample must fit with one sinusoid per tile");

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
  const float e = expf(-fabsf(x));
  return (x >= 0.0f) ? 1.0f / (1.0f + e) : e / (1.0f + e);
}
__device__ __forceinline__ float midi_to_hz(float m) { return 440.0f * exp2f((m - 69.0f) * (1.0f / 12.0f)); }

// ---- the frequency scale functions ------------------------------------------------------------------------------------
// unit_to_hz(u, lo, hi) = midi_to_hz(m_lo + (m_hi - m_lo) u) with m = hz_to_midi of the two bounds: host-side constants.
//   frequencies_sigmoid: sum over the `depth` terms of unit_to_hz(sigmoid(x_i), lo_i, hi_i)   (midi_min / midi_span per term)
//   frequencies_softmax: unit_to_hz(sum_i softmax(x)_i i / (depth - 1), hz_min, hz_max)        (entry 0 only)
struct FreqScale {
  int mode;                    // 0: the input is in Hz already, 1: sigmoid, 2: softmax
  int depth;
  float midi_min[kMaxDepth], midi_span[kMaxDepth];
};

static double hz_to_midi_host(double hz) { return hz <= 0.0 ? 0.0 : 12.0 * (log2(hz) - log2(440.0)) + 69.0; }

static int make_freq_scale(unsigned flags, int depth, float hz_min, float hz_max, FreqScale* s) {
  const bool sig = (flags & DDSP_SIN_FREQ_SIGMOID) != 0, soft = (flags & DDSP_SIN_FREQ_SOFTMAX) != 0;
  s->mode = sig ? 1 : (soft ? 2 : 0);
  s->depth = s->mode ? depth : 1;
  for (int i = 0; i < kMaxDepth; ++i) { s->midi_min[i] = 0.0f; s->midi_span[i] = 0.0f; }
  if (sig && soft) return DDSP_ERR_UNSUPPORTED;
  if (s->mode == 0) return DDSP_OK;
  if (depth < 1) return DDSP_ERR_BAD_SHAPE;
  if (soft) {
    const double lo = hz_to_midi_host((double)hz_min), hi = hz_to_midi_host((double)hz_max);
    s->midi_min[0] = (float)lo; s->midi_span[0] = (float)(hi - lo);
    return DDSP_OK;
  }
  if (depth > kMaxDepth) return DDSP_ERR_UNSUPPORTED;
  // ddsp/core.py:487-505: the range is split in `depth` parts, each a constant factor smaller than the one before
  double remainder = (double)hz_max - (double)hz_min;
  const double scale_factor = pow(remainder, 1.0 / (double)depth);
  for (int i = 0; i < depth; ++i) {
    double hi, lo;
    if (i == depth - 1) { hi = remainder; lo = (double)hz_min; }
    else { hi = remainder * (1.0 - 1.0 / scale_factor); lo = 0.0; remainder -= hi; }
    const double m_lo = hz_to_midi_host(lo), m_hi = hz_to_midi_host(hi);
    s->midi_min[i] = (float)m_lo; s->midi_span[i] = (float)(m_hi - m_lo);
  }
  return DDSP_OK;
}

__device__ __forceinline__ float softmax_unit(const float* __restrict__ x, int D, float& denom, float& mx) {
  mx = x[0];
  for (int i = 1; i < D; ++i) mx = fmaxf(mx, x[i]);
  float num = 0.0f;
  denom = 0.0f;
  const float step = D > 1 ? 1.0f / (float)(D - 1) : 0.0f;
  for (int i = 0; i < D; ++i) {
    const float e = expf(x[i] - mx);
    denom += e;
    num = fmaf(e, (float)i * step, num);
  }
  return num / denom;
}

// One thread per (row, sinusoid).  amps may be null (the scale functions on their own).  BWD: grad_ctl_* -> grad_*.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void sin_controls_kernel(const float* __restrict__ amps /*[R,K]*/,
                                                                const float* __restrict__ freqs /*[R,K*D]*/,
                                                                const float* __restrict__ g_ctl_amp, const float* __restrict__ g_ctl_freq,
                                                                float* __restrict__ out_amp, float* __restrict__ out_freq, size_t total,
                                                                float nyquist, unsigned flags, FreqScale sc) {
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int D = sc.depth;
  const float* __restrict__ x = freqs + idx * (size_t)D;
  float f;
  float unit = 0.0f, denom = 1.0f, mx = 0.0f;
  if (sc.mode == 0) {
    f = x[0];
  } else if (sc.mode == 1) {
    f = 0.0f;
    for (int i = 0; i < D; ++i) f += midi_to_hz(fmaf(sc.midi_span[i], sigmoid(x[i]), sc.midi_min[i]));
  } else {
    unit = softmax_unit(x, D, denom, mx);
    f = midi_to_hz(fmaf(sc.midi_span[0], unit, sc.midi_min[0]));
  }
  const bool masked = (flags & DDSP_SIN_MASK_NYQUIST) && f >= nyquist;
  if (!BWD) {
    out_freq[idx] = f;
    if (amps) {
      const float a = (flags & DDSP_SIN_AMP_EXP_SIGMOID) ? exp_sigmoid(amps[idx]) : amps[idx];
      out_amp[idx] = masked ? 0.0f : a;
    }
  } else {
    if (amps) {
      const float g = g_ctl_amp[idx];
      out_amp[idx] = masked ? 0.0f : ((flags & DDSP_SIN_AMP_EXP_SIGMOID) ? g * exp_sigmoid_grad(amps[idx]) : g);
    }
    const float g = g_ctl_freq ? g_ctl_freq[idx] : 0.0f;
    float* __restrict__ gx = out_freq + idx * (size_t)D;
    if (sc.mode == 0) {
      gx[0] = g;
    } else if (sc.mode == 1) {
      for (int i = 0; i < D; ++i) {
        const float s = sigmoid(x[i]);
        const float hz = midi_to_hz(fmaf(sc.midi_span[i], s, sc.midi_min[i]));
        gx[i] = g * hz * kLn2Over12 * sc.midi_span[i] * s * (1.0f - s);
      }
    } else {
      const float k = g * f * kLn2Over12 * sc.midi_span[0];
      const float step = D > 1 ? 1.0f / (float)(D - 1) : 0.0f;
      for (int i = 0; i < D; ++i) gx[i] = k * (expf(x[i] - mx) / denom) * ((float)i * step - unit);
    }
  }
}

// ---- elementwise conversions (ddsp/core.py:219-348) ----------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void unit_convert_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n, int op,
                                                                float p0, float p1) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float x = in[i];
  float y;
  switch (op) {
    case DDSP_CONVERT_MIDI_TO_HZ: y = midi_to_hz(x); break;
    case DDSP_CONVERT_MIDI_TO_HZ_ZERO_SILENCE: y = (x == 0.0f) ? 0.0f : midi_to_hz(x); break;
    case DDSP_CONVERT_HZ_TO_MIDI: y = (x <= 0.0f) ? 0.0f : 12.0f * (log2f(x) - log2f(440.0f)) + 69.0f; break;
    case DDSP_CONVERT_UNIT_TO_MIDI: y = p0 + (p1 - p0) * x; break;
    case DDSP_CONVERT_UNIT_TO_MIDI_CLIP: y = p0 + (p1 - p0) * min_keep_nan(max_keep_nan(x, 0.0f), 1.0f); break;
    case DDSP_CONVERT_MIDI_TO_UNIT: y = (x - p0) / (p1 - p0); break;
    case DDSP_CONVERT_MIDI_TO_UNIT_CLIP: y = min_keep_nan(max_keep_nan((x - p0) / (p1 - p0), 0.0f), 1.0f); break;
    case DDSP_CONVERT_LOG_FLOOR: { const float m = max_keep_nan(x, p1); y = logf(m <= 0.0f ? 1e-5f : m) / p0; break; }   // core.log10(tf.maximum(amin, x)): p0 = ln 10, p1 = amin
    default: y = logf(x <= 0.0f ? p1 : x) / p0; break;                  // DDSP_CONVERT_LOGB: p0 = safe log of the base, p1 = eps
  }
  out[i] = y;
}

// ---- synthesis ---------------------------------------------------------------------------------------------------------------
struct SinArgs {
  int F, K, N, hop;          // hop = N / F
  int KT;                    // sinusoids per LDS tile of sin_synth_kernel
  float sample_rate, nyquist;
  int linear;                // amplitude envelope: 0 'window', 1 'linear'
};

// Hz-samples of frame j: sum over r = 0 .. hop - 1 of f_j + (f_{j+1} - f_j) r / hop
__device__ __forceinline__ double frame_hz_samples(const float* __restrict__ f, int j, int F, int K, int hop) {
  const double fa = (double)f[(size_t)j * K], fb = (double)f[(size_t)min(j + 1, F - 1) * K];
  return (double)hop * fa + (fb - fa) * (0.5 * (double)(hop - 1));
}

// phase0[b, j, k]: cycles accumulated before frame j, wrapped to [0, 1).  Block (tile of 16 sinusoids, row).
__global__ __launch_bounds__(kThreads) void sin_prefix_kernel(const float* __restrict__ freqs /*[B,F,K]*/, float* __restrict__ phase0 /*[B,F,K]*/,
                                                              SinArgs p) {
  __shared__ double s_tot[kSegs][kLanesK];
  const int kk = threadIdx.x % kLanesK, seg = threadIdx.x / kLanesK;
  const int k = blockIdx.x * kLanesK + kk, b = blockIdx.y;
  const bool live = k < p.K;
  const float* __restrict__ fb = freqs + (size_t)b * p.F * p.K + (live ? k : 0);
  float* __restrict__ pb = phase0 + (size_t)b * p.F * p.K + (live ? k : 0);
  const int per = (p.F + kSegs - 1) / kSegs;
  const int j_lo = min(seg * per, p.F), j_hi = min(j_lo + per, p.F);
  double local = 0.0;
  if (live)
    for (int j = j_lo; j < j_hi; ++j) local += frame_hz_samples(fb, j, p.F, p.K, p.hop);
  s_tot[seg][kk] = local;
  __syncthreads();
  if (!live) return;
  double before = 0.0;
  for (int s = 0; s < seg; ++s) before += s_tot[s][kk];
  const double inv_sr = 1.0 / (double)p.sample_rate;
  for (int j = j_lo; j < j_hi; ++j) {
    const double cyc = before * inv_sr;
    pb[(size_t)j * p.K] = (float)(cyc - floor(cyc));
    before += frame_hz_samples(fb, j, p.F, p.K, p.hop);
  }
}

struct Coef {
  double c0, c1, c2;          // phase(r) = c0 + (r + 1) c1 + (r (r + 1) / 2) c2, cycles
  float a0, da;               // amplitude(r) = a0 + w(r) da
  float f0, df;               // frequency(r) = f0 + (r / hop) df, for the audio-rate Nyquist test
};

__device__ __forceinline__ Coef make_coef(float aj, float ajn, float fj, float fjn, float ph0, double inv_sr, double inv_hop,
                                          float nyquist, bool& mixed) {
  Coef c;
  c.c0 = (double)ph0;
  c.c1 = (double)fj * inv_sr;
  c.c2 = ((double)fjn - (double)fj) * inv_sr * inv_hop;
  const bool above_j = fj >= nyquist, above_n = fjn >= nyquist;
  mixed = above_j != above_n;
  const bool silent = above_j && above_n;            // every interpolated value is at or above Nyquist
  c.a0 = silent ? 0.0f : aj;
  c.da = silent ? 0.0f : ajn - aj;
  c.f0 = fj;
  c.df = fjn - fj;
  return c;
}

__device__ __forceinline__ float wrapped_phase(const Coef& c, double r1, double tri) {
  const double ph = fma(tri, c.c2, fma(r1, c.c1, c.c0));
  return (float)__builtin_amdgcn_fract(ph);
}

template <bool MASK>
__device__ __forceinline__ void synth_tile(const Coef* __restrict__ s_coef, int KT, int kt, const int (&row)[kSamplesPerThread],
                                           const double (&r1)[kSamplesPerThread], const double (&tri)[kSamplesPerThread],
                                           const float (&w)[kSamplesPerThread], const float (&lerp)[kSamplesPerThread], float nyquist,
                                           float (&acc)[kSamplesPerThread]) {
  for (int kk = 0; kk < kt; ++kk) {
#pragma unroll
    for (int s = 0; s < kSamplesPerThread; ++s) {
      const Coef c = s_coef[row[s] * KT + kk];
      const float sn = __builtin_amdgcn_sinf(wrapped_phase(c, r1[s], tri[s]));
      float a = fmaf(w[s], c.da, c.a0);
      if (MASK) {
        if (fmaf(c.df, lerp[s], c.f0) >= nyquist) a = 0.0f;
      }
      acc[s] = fmaf(a, sn, acc[s]);
    }
  }
}

// Block (run of kChunk samples, row).  amps / freqs are CONTROLS [B,F,K]; phase0 from sin_prefix_kernel.
__global__ __launch_bounds__(kThreads) void sin_synth_kernel(const float* __restrict__ amps, const float* __restrict__ freqs,
                                                             const float* __restrict__ phase0, float* __restrict__ out /*[B,N]*/, SinArgs p) {
  __shared__ Coef s_coef[kMaxEntries];
  __shared__ int s_mixed;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * kChunk, t_end = min(t0 + kChunk, p.N);
  const int j_lo = t0 / p.hop, j_hi = (t_end - 1) / p.hop;
  const int n_frames = j_hi - j_lo + 1;
  const size_t row0 = (size_t)b * p.F * p.K;
  const double inv_sr = 1.0 / (double)p.sample_rate, inv_hop = 1.0 / (double)p.hop;

  int row[kSamplesPerThread];
  double r1[kSamplesPerThread], tri[kSamplesPerThread];
  float w[kSamplesPerThread], lerp[kSamplesPerThread], acc[kSamplesPerThread];
#pragma unroll
  for (int s = 0; s < kSamplesPerThread; ++s) {
    const int t = min(t0 + (int)threadIdx.x + s * kThreads, t_end - 1);      // (a thread past the end repeats the last sample, unstored)
    const int j = t / p.hop, r = t - j * p.hop;
    row[s] = j - j_lo;
    r1[s] = (double)(r + 1);
    tri[s] = 0.5 * (double)r * (double)(r + 1);
    lerp[s] = (float)r / (float)p.hop;
    w[s] = p.linear ? lerp[s] : 0.5f - 0.5f * cospif(lerp[s]);               // the rising half of the periodic Hann(2 hop)
    acc[s] = 0.0f;
  }
  if (threadIdx.x == 0) s_mixed = 0;
  for (int k0 = 0; k0 < p.K; k0 += p.KT) {
    const int kt = min(p.KT, p.K - k0);
    __syncthreads();                                   // the tile before this one has been consumed
    for (int e = threadIdx.x; e < n_frames * kt; e += kThreads) {
      const int jl = e / kt, kk = e - jl * kt;
      const int j = j_lo + jl, jn = min(j + 1, p.F - 1);
      const size_t ia = row0 + (size_t)j * p.K + k0 + kk, ib = row0 + (size_t)jn * p.K + k0 + kk;
      bool mixed;
      s_coef[jl * p.KT + kk] = make_coef(amps[ia], amps[ib], freqs[ia], freqs[ib], phase0[ia], inv_sr, inv_hop, p.nyquist, mixed);
      if (mixed) s_mixed = 1;
    }
    __syncthreads();
    if (s_mixed) synth_tile<true>(s_coef, p.KT, kt, row, r1, tri, w, lerp, p.nyquist, acc);
    else synth_tile<false>(s_coef, p.KT, kt, row, r1, tri, w, lerp, p.nyquist, acc);
  }
#pragma unroll
  for (int s = 0; s < kSamplesPerThread; ++s) {
    const int t = t0 + (int)threadIdx.x + s * kThreads;
    if (t < t_end) out[(size_t)b * p.N + t] = acc[s];
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------
// Per (row, frame, sinusoid), with g the incoming gradient, m the audio-rate mask, a the amplitude envelope, w the window weight:
//   p_lo = sum g m sin (1 - w)     p_hi = sum g m sin w                           (-> the amplitudes of frame j and j + 1)
//   c_sum = sum c    c_r1 = sum c (r + 1)    c_tri = sum c r (r + 1) / 2          with c = g a m cos(phase) 2 pi / sr
struct BwdSums { float* p_lo; float* p_hi; float* c_sum; float* c_r1; float* c_tri; };     // [B,F,K] each

__global__ __launch_bounds__(kThreads) void sin_bwd_sums_kernel(const float* __restrict__ amps, const float* __restrict__ freqs,
                                                                const float* __restrict__ phase0, const float* __restrict__ gout /*[B,N]*/,
                                                                BwdSums out, SinArgs p) {
  __shared__ float s_w[kRChunk], s_lerp[kRChunk];
  const int b = blockIdx.y;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  const bool live = e < p.F * p.K;
  const int j = live ? e / p.K : 0, k = live ? e - j * p.K : 0;
  const int jn = min(j + 1, p.F - 1);
  const size_t row0 = (size_t)b * p.F * p.K;
  const size_t ia = row0 + (size_t)j * p.K + k, ib = row0 + (size_t)jn * p.K + k;
  bool mixed;
  const Coef c = make_coef(amps[ia], amps[ib], freqs[ia], freqs[ib], phase0[ia], 1.0 / (double)p.sample_rate, 1.0 / (double)p.hop,
                           p.nyquist, mixed);
  const bool silent = c.f0 >= p.nyquist && !mixed;           // masked throughout: every sum is zero
  const float* __restrict__ gb = gout + (size_t)b * p.N + (size_t)j * p.hop;
  float p_lo = 0.0f, p_hi = 0.0f, c_sum = 0.0f, c_r1 = 0.0f, c_tri = 0.0f;
  for (int rc = 0; rc < p.hop; rc += kRChunk) {
    const int n = min(kRChunk, p.hop - rc);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const float l = (float)(rc + i) / (float)p.hop;
      s_lerp[i] = l;
      s_w[i] = p.linear ? l : 0.5f - 0.5f * cospif(l);
    }
    __syncthreads();
    if (!live || silent) continue;
    double r1 = (double)(rc + 1), tri = 0.5 * (double)rc * (double)(rc + 1);
    for (int i = 0; i < n; ++i) {
      const float x = wrapped_phase(c, r1, tri);
      const float sn = __builtin_amdgcn_sinf(x), cs = __builtin_amdgcn_cosf(x);
      const float w = s_w[i];
      float g = gb[rc + i];
      if (mixed && fmaf(c.df, s_lerp[i], c.f0) >= p.nyquist) g = 0.0f;
      const float gs = g * sn;
      p_lo = fmaf(gs, 1.0f - w, p_lo);
      p_hi = fmaf(gs, w, p_hi);
      const float cv = g * fmaf(w, c.da, c.a0) * cs;
      c_sum += cv;
      c_r1 = fmaf(cv, (float)r1, c_r1);
      c_tri = fmaf(cv, (float)tri, c_tri);
      tri += r1;
      r1 += 1.0;
    }
  }
  if (!live) return;
  const float two_pi_over_sr = 6.283185307179586f / p.sample_rate;
  out.p_lo[ia] = p_lo;
  out.p_hi[ia] = p_hi;
  out.c_sum[ia] = c_sum * two_pi_over_sr;
  out.c_r1[ia] = c_r1 * two_pi_over_sr;
  out.c_tri[ia] = c_tri * two_pi_over_sr;
}

// dL/d amplitudes[j] = p_lo[j] + p_hi[j - 1] (+ p_hi[j] on the held last frame).
// dL/d frequencies: dL/d f_env[t] = S(t) = sum over n >= t of c[n]; frame j's frequency weighs S by 1 - r / hop over its own samples
// and by r / hop over frame j - 1's (both on the held last frame).  With `later` the sum of c over the frames after j:
//   sum_r (1 - r / hop) S = c_r1 - c_tri / hop + later (hop + 1) / 2          sum_r (r / hop) S = c_tri / hop + later (hop - 1) / 2
__global__ __launch_bounds__(kThreads) void sin_bwd_scan_kernel(BwdSums in, float* __restrict__ gamps /*[B,F,K]*/, float* __restrict__ gfreqs,
                                                                SinArgs p) {
  __shared__ double s_tot[kSegs][kLanesK];
  const int kk = threadIdx.x % kLanesK, seg = threadIdx.x / kLanesK;
  const int k = blockIdx.x * kLanesK + kk, b = blockIdx.y;
  const bool live = k < p.K;
  const size_t base = (size_t)b * p.F * p.K + (live ? k : 0);
  const int per = (p.F + kSegs - 1) / kSegs;
  const int j_lo = min(seg * per, p.F), j_hi = min(j_lo + per, p.F);
  double local = 0.0;
  if (live)
    for (int j = j_lo; j < j_hi; ++j) local += (double)in.c_sum[base + (size_t)j * p.K];
  s_tot[seg][kk] = local;
  __syncthreads();
  if (!live) return;
  double later = 0.0;
  for (int s = kSegs - 1; s > seg; --s) later += s_tot[s][kk];
  const double inv_hop = 1.0 / (double)p.hop, w_own = 0.5 * (double)(p.hop + 1), w_next = 0.5 * (double)(p.hop - 1);
  for (int j = j_hi - 1; j >= j_lo; --j) {
    const size_t o = base + (size_t)j * p.K;
    const double tri = (double)in.c_tri[o] * inv_hop;
    double gf = (double)in.c_r1[o] - tri + later * w_own;
    float ga = in.p_lo[o];
    if (j == p.F - 1) { gf += tri + later * w_next; ga += in.p_hi[o]; }
    later += (double)in.c_sum[o];                               // now the sum over the frames after j - 1
    if (j > 0) {
      const size_t q = o - (size_t)p.K;
      gf += (double)in.c_tri[q] * inv_hop + later * w_next;
      ga += in.p_hi[q];
    }
    gamps[o] = ga;
    gfreqs[o] = (float)gf;
  }
}

static inline size_t align_up(size_t n, size_t a) { return (n + a - 1) / a * a; }
static inline size_t plane_bytes(int B, int F, int K) { return align_up((size_t)B * F * K * sizeof(float), 16); }

static int check_shape(int B, int F, int K, int N, float sample_rate) {
  if (B <= 0 || F <= 0 || K <= 0 || N <= 0 || B > 65535 || !(sample_rate > 0.0f)) return DDSP_ERR_BAD_SHAPE;
  if ((size_t)F * K > (size_t)0x7fffffff) return DDSP_ERR_BAD_SHAPE;
  if (N % F != 0) return DDSP_ERR_UNSUPPORTED;         // the closed forms need whole frames: the caller takes the materialised chain
  return DDSP_OK;
}

static SinArgs make_args(int F, int K, int N, float sample_rate, unsigned flags) {
  SinArgs p;
  p.F = F; p.K = K; p.N = N; p.hop = N / F;
  p.sample_rate = sample_rate; p.nyquist = sample_rate / 2.0f;
  p.linear = (flags & DDSP_SIN_AMP_LINEAR) ? 1 : 0;
  // the most frames a run of kChunk samples starting at a multiple of kChunk touches
  int frames = (kChunk % p.hop == 0) ? kChunk / p.hop : (kChunk - 1) / p.hop + 2;
  if (frames > F) frames = F;
  p.KT = kMaxEntries / frames;
  if (p.KT > K) p.KT = K;
  return p;
}

static unsigned blocks_for(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

static int launch_controls(const float* amps, const float* freqs, float* ctl_amp, float* ctl_freq, size_t rows, int K, int depth,
                           float hz_min, float hz_max, float sample_rate, unsigned flags, hipStream_t st) {
  FreqScale sc;
  const int rc = make_freq_scale(flags, depth, hz_min, hz_max, &sc);
  if (rc != DDSP_OK) return rc;
  const size_t total = rows * (size_t)K;
  if (total > (size_t)0x7fffffff * kThreads) return DDSP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL((sin_controls_kernel<false>), dim3(blocks_for(total)), dim3(kThreads), 0, st, amps, freqs, (const float*)nullptr,
                     (const float*)nullptr, ctl_amp, ctl_freq, total, sample_rate / 2.0f, flags, sc);
  return check_launch();
}

static int launch_signal(const float* ctl_amp, const float* ctl_freq, float* audio, float* phase0, int B, const SinArgs& p,
                         hipStream_t st) {
  hipLaunchKernelGGL(sin_prefix_kernel, dim3((unsigned)((p.K + kLanesK - 1) / kLanesK), (unsigned)B), dim3(kThreads), 0, st, ctl_freq,
                     phase0, p);
  hipEvent_t ev0, ev1;
  profile_kernel_events(kSinSynth, &ev0, &ev1);
  hipExtLaunchKernelGGL(sin_synth_kernel, dim3((unsigned)((p.N + kChunk - 1) / kChunk), (unsigned)B), dim3(kThreads), 0, st, ev0, ev1, 0,
                        ctl_amp, ctl_freq, (const float*)phase0, audio, p);
  return check_launch();
}

constexpr unsigned kScaleFlags = DDSP_SIN_AMP_EXP_SIGMOID | DDSP_SIN_FREQ_SIGMOID | DDSP_SIN_FREQ_SOFTMAX | DDSP_SIN_MASK_NYQUIST;

}  // namespace sinusoidal
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::sinusoidal;

extern "C" int ddsp_sinusoidal_controls_f32(const float* amplitudes, const float* frequencies, float* ctl_amplitudes,
                                            float* ctl_frequencies, size_t rows, int K, int depth, float hz_min, float hz_max,
                                            float sample_rate, unsigned flags, void* stream) {
  if (!frequencies || !ctl_frequencies || ((amplitudes == nullptr) != (ctl_amplitudes == nullptr))) return DDSP_ERR_NULL_POINTER;
  if (rows == 0 || K <= 0 || !(sample_rate > 0.0f)) return DDSP_ERR_BAD_SHAPE;
  return launch_controls(amplitudes, frequencies, ctl_amplitudes, ctl_frequencies, rows, K, depth, hz_min, hz_max, sample_rate, flags,
                         (hipStream_t)stream);
}

extern "C" int ddsp_sinusoidal_controls_backward_f32(const float* amplitudes, const float* frequencies, const float* grad_ctl_amplitudes,
                                                     const float* grad_ctl_frequencies, float* grad_amplitudes, float* grad_frequencies,
                                                     size_t rows, int K, int depth, float hz_min, float hz_max, float sample_rate,
                                                     unsigned flags, void* stream) {
  if (!frequencies || !grad_frequencies) return DDSP_ERR_NULL_POINTER;
  if ((amplitudes == nullptr) != (grad_amplitudes == nullptr) || (amplitudes == nullptr) != (grad_ctl_amplitudes == nullptr))
    return DDSP_ERR_NULL_POINTER;
  if (rows == 0 || K <= 0 || !(sample_rate > 0.0f)) return DDSP_ERR_BAD_SHAPE;
  FreqScale sc;
  const int rc = make_freq_scale(flags, depth, hz_min, hz_max, &sc);
  if (rc != DDSP_OK) return rc;
  const size_t total = rows * (size_t)K;
  if (total > (size_t)0x7fffffff * kThreads) return DDSP_ERR_BAD_SHAPE;
  hipLaunchKernelGGL((sin_controls_kernel<true>), dim3(blocks_for(total)), dim3(kThreads), 0, (hipStream_t)stream, amplitudes, frequencies,
                     grad_ctl_amplitudes, grad_ctl_frequencies, grad_amplitudes, grad_frequencies, total, sample_rate / 2.0f, flags, sc);
  return check_launch();
}

extern "C" int ddsp_unit_convert_f32(const float* in, float* out, size_t n, int op, float p0, float p1, void* stream) {
  if (!in || !out) return DDSP_ERR_NULL_POINTER;
  if (n == 0 || n > (size_t)0x7fffffff * kThreads) return DDSP_ERR_BAD_SHAPE;
  if (op < DDSP_CONVERT_MIDI_TO_HZ || op > DDSP_CONVERT_LOG_FLOOR) return DDSP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(unit_convert_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, in, out, n, op, p0, p1);
  return check_launch();
}

extern "C" size_t ddsp_sinusoidal_workspace_bytes(int B, int F, int K, int N) {
  (void)N;
  if (B <= 0 || F <= 0 || K <= 0) return 0;
  return 3 * plane_bytes(B, F, K);                      // the controls (when the inputs are raw) and the frames' start phases
}

extern "C" int ddsp_sinusoidal_signal_f32(const float* amplitudes, const float* frequencies, float* audio, void* workspace,
                                          size_t workspace_bytes, int B, int F, int K, int N, float sample_rate, unsigned flags,
                                          void* stream) {
  if (!amplitudes || !frequencies || !audio || !workspace) return DDSP_ERR_NULL_POINTER;
  const int rc = check_shape(B, F, K, N, sample_rate);
  if (rc != DDSP_OK) return rc;
  if (flags & kScaleFlags) return DDSP_ERR_UNSUPPORTED;           // the inputs of this entry are controls
  if (workspace_bytes < ddsp_sinusoidal_workspace_bytes(B, F, K, N) || ((uintptr_t)workspace & 15)) return DDSP_ERR_WORKSPACE;
  const SinArgs p = make_args(F, K, N, sample_rate, flags);
  return launch_signal(amplitudes, frequencies, audio, (float*)workspace, B, p, (hipStream_t)stream);
}

extern "C" int ddsp_sinusoidal_f32(const float* amplitudes, const float* frequencies, float* audio, float* ctl_amplitudes,
                                   float* ctl_frequencies, void* workspace, size_t workspace_bytes, int B, int F, int K, int N, int depth,
                                   float hz_min, float hz_max, float sample_rate, unsigned flags, void* stream) {
  if (!amplitudes || !frequencies || !audio || !workspace) return DDSP_ERR_NULL_POINTER;
  if ((ctl_amplitudes == nullptr) != (ctl_frequencies == nullptr)) return DDSP_ERR_NULL_POINTER;
  const int rc = check_shape(B, F, K, N, sample_rate);
  if (rc != DDSP_OK) return rc;
  if (workspace_bytes < ddsp_sinusoidal_workspace_bytes(B, F, K, N) || ((uintptr_t)workspace & 15)) return DDSP_ERR_WORKSPACE;
  const size_t plane = plane_bytes(B, F, K);
  char* ws = (char*)workspace;
  float* phase0 = (float*)ws;
  float* ctl_a = ctl_amplitudes ? ctl_amplitudes : (float*)(ws + plane);
  float* ctl_f = ctl_frequencies ? ctl_frequencies : (float*)(ws + 2 * plane);
  const hipStream_t st = (hipStream_t)stream;
  const int rc2 = launch_controls(amplitudes, frequencies, ctl_a, ctl_f, (size_t)B * F, K, depth, hz_min, hz_max, sample_rate, flags, st);
  if (rc2 != DDSP_OK) return rc2;
  const SinArgs p = make_args(F, K, N, sample_rate, flags);
  return launch_signal(ctl_a, ctl_f, audio, phase0, B, p, st);
}

extern "C" size_t ddsp_sinusoidal_backward_workspace_bytes(int B, int F, int K, int N) {
  (void)N;
  if (B <= 0 || F <= 0 || K <= 0) return 0;
  return 10 * plane_bytes(B, F, K);       // controls (2), start phases, five sums, the two control gradients
}

extern "C" int ddsp_sinusoidal_backward_f32(const float* amplitudes, const float* frequencies, const float* grad_audio,
                                            float* grad_amplitudes, float* grad_frequencies, void* workspace, size_t workspace_bytes,
                                            int B, int F, int K, int N, int depth, float hz_min, float hz_max, float sample_rate,
                                            unsigned flags, void* stream) {
  if (!amplitudes || !frequencies || !grad_audio || !grad_amplitudes || !grad_frequencies || !workspace) return DDSP_ERR_NULL_POINTER;
  const int rc = check_shape(B, F, K, N, sample_rate);
  if (rc != DDSP_OK) return rc;
  if (workspace_bytes < ddsp_sinusoidal_backward_workspace_bytes(B, F, K, N) || ((uintptr_t)workspace & 15)) return DDSP_ERR_WORKSPACE;
  FreqScale sc;
  const int rcs = make_freq_scale(flags, depth, hz_min, hz_max, &sc);
  if (rcs != DDSP_OK) return rcs;
  const size_t plane = plane_bytes(B, F, K);
  char* ws = (char*)workspace;
  float* phase0 = (float*)ws;
  const bool raw = (flags & kScaleFlags) != 0;
  const float* ctl_a = amplitudes;
  const float* ctl_f = frequencies;
  const hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)B * F * K;
  if (raw) {
    float* a = (float*)(ws + plane);
    float* f = (float*)(ws + 2 * plane);
    hipLaunchKernelGGL((sin_controls_kernel<false>), dim3(blocks_for(total)), dim3(kThreads), 0, st, amplitudes, frequencies,
                       (const float*)nullptr, (const float*)nullptr, a, f, total, sample_rate / 2.0f, flags, sc);
    ctl_a = a; ctl_f = f;
  }
  BwdSums sums;
  sums.p_lo = (float*)(ws + 3 * plane); sums.p_hi = (float*)(ws + 4 * plane); sums.c_sum = (float*)(ws + 5 * plane);
  sums.c_r1 = (float*)(ws + 6 * plane); sums.c_tri = (float*)(ws + 7 * plane);
  float* g_ctl_a = raw ? (float*)(ws + 8 * plane) : grad_amplitudes;
  float* g_ctl_f = raw ? (float*)(ws + 9 * plane) : grad_frequencies;
  const SinArgs p = make_args(F, K, N, sample_rate, flags);
  const dim3 scan_grid((unsigned)((K + kLanesK - 1) / kLanesK), (unsigned)B);
  hipLaunchKernelGGL(sin_prefix_kernel, scan_grid, dim3(kThreads), 0, st, ctl_f, phase0, p);
  hipEvent_t ev0, ev1;
  profile_kernel_events(kSinBwdSums, &ev0, &ev1);
  hipExtLaunchKernelGGL(sin_bwd_sums_kernel, dim3(blocks_for((size_t)F * K), (unsigned)B), dim3(kThreads), 0, st, ev0, ev1, 0, ctl_a, ctl_f,
                        (const float*)phase0, grad_audio, sums, p);
  hipLaunchKernelGGL(sin_bwd_scan_kernel, scan_grid, dim3(kThreads), 0, st, sums, g_ctl_a, g_ctl_f, p);
  if (raw)
    hipLaunchKernelGGL((sin_controls_kernel<true>), dim3(blocks_for(total)), dim3(kThreads), 0, st, amplitudes, frequencies,
                       (const float*)g_ctl_a, (const float*)g_ctl_f, grad_amplitudes, grad_frequencies, total, sample_rate / 2.0f, flags,
                       sc);
  return check_launch();
}
