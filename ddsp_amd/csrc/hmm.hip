// losses.HmmTranscriber (ddsp/losses.py:246-345) for gfx950: the log-likelihood of tfp's HiddenMarkovModel.log_prob, its
// gradient in the observations, and the Viterbi path of posterior_mode.
//
// The transition matrix the constructor builds is other * 1 + (hold - other) * I, so one step of the forward algorithm is
//     alpha'[s] = (other * sum_i alpha[i] + (hold - other) * alpha[s]) * exp(obs[t, s])
// and one Viterbi step (hold >= other) is max(v[s] + log hold, max_i v[i] + log other) + obs[t, s]: O(states) a step, and
// nothing of size [states, states] or [rows, steps, states, states] exists.  The chain over the steps is serial and latency
// bound, so a block owns a row and walks it; a thread holds the states tid, tid + NT, tid + 2 NT, tid + 3 NT in registers.
//   * states <= 256: NT = 64, ONE wavefront.  The one reduction a step has on its chain is six DPP adds and a v_readlane
//     (common.h): no LDS, no barrier.
//   * states <= 1024: NT = 256, the wavefronts' results meet in LDS (two barriers a reduction).
// The observations (pitch, amps) of 64 steps are loaded by the 64 lanes at once, the chunk after it while this one is worked
// on, and handed out a step at a time by v_readlane: no global load sits on the chain.
//
// obs[t, s] = log N(pitch_t; loc_s, scale_s) + log N(amps_t; ...) is evaluated from the two scalars of the step, RELATIVE to
// its maximum over the states m_t, which has a closed form (state 0, or the state nearest the pitch): no reduction.  m_t is
// taken in fp64; obs[t, s] - m_t for an "on" state is (m_on - m_t) - (s* - s) ((p - s) + (p - s*)) / (2 std^2), a product of
// small differences instead of a difference of large squares.  So amps = 50 or pitch = -300 shift m_t and leave the
// exponentials in [0, 1] with at least one of them 1: no underflow of a whole step, no NaN.
//
//   1. log_prob   the forward variables are rescaled every step by the power of two that brings their sum into [1/2, 1):
//                 exact, and its exponent is counted in an INTEGER.  log_prob = sum_t m_t (fp64, in step order)
//                 + ln 2 * exponents + log(last sum) - log(states): no fp32 number ever grows with the clip's length.
//   2. backward   d log_prob / d pitch_t = -sum_s gamma[t, s] (pitch_t - loc_s) / scale_s^2 (amps alike), gamma the
//                 posterior marginals.  The kernel runs the forward sweep again, storing the rescaled forward variables in
//                 the workspace ([rows, steps, states] floats; a thread reads back only what it wrote), then the backward
//                 recursion, which has the same form: beta[i] = other * sum_s e[s] beta'[s] + (hold - other) e[i] beta'[i].
//                 Thread 0 writes the two gradients of a step: no atomics, every element written once.  All "on" states
//                 share the amps model, so the amps gradient needs gamma[t, 0] alone.
//   3. Viterbi    v is kept relative to its maximum.  For the back trace a step needs one "stayed" bit per state and the
//                 arg-max of the step before it; the bits are kept TRANSPOSED, a 32-bit word per state and 32 steps
//                 (accumulated in a register, stored once in 32 steps), so the back trace finds the last step at which the
//                 current state was entered with one load and a count of leading zeros per 32 steps, and fills the run in
//                 parallel.  Workspace: [rows, ceil(steps / 32), states] words + [rows, steps] arg-maxes, in global memory
//                 for any number of steps (16 KB + 4 KB a row at 1000 x 128).  Ties go to the lowest index, as argmax does.
//
// Bounds (beyond them DDSP_ERR_UNSUPPORTED): 2 <= states <= 1024; hold >= other > 0.
// With `rows` blocks of one wavefront most of the chip idles at batch 32: accepted; a scan that is
// parallel in time is not built.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "common.h"
#include "launch.h"

namespace ddsp {
namespace hmm {

constexpr int kQ = 4;                     // states a thread holds
constexpr int kMaxStates = 1024;
constexpr int kChunk = 64;                // steps whose observations a wavefront holds, one per lane

struct Model {
  int n;
  float hmo, other, log_hold, log_other;          // hold - other, other; their logarithms for Viterbi
  float half_ivar;                                // 1 / (2 midi_std^2)
  float ivar_on_p, ivar_off_p, ivar_on_a, ivar_off_a, loc_off_p, a_on, a_off;      // the gradients' 1 / scale^2 and centres
  double inv_std, inv_n, inv_s_on, inv_s_off, loc_off, a_on_d, a_off_d, k_on, k_off, log_n;
};

// what a step's two scalars give: s* = the "on" state nearest the pitch, m = max_s obs[t, s], and m_on - m, m_off - m
struct Obs { float p, a, sstar, c_on, c_off; double m; };

__device__ __forceinline__ Obs observe(const Model& M, float p, float a) {
  Obs o;
  o.p = p; o.a = a;
  o.sstar = fminf(fmaxf(rintf(p), 1.0f), (float)(M.n - 1));
  const double zp = ((double)p - (double)o.sstar) * M.inv_std, za = ((double)a - M.a_on_d) * M.inv_s_on;
  const double yp = ((double)p - M.loc_off) * M.inv_n, ya = ((double)a - M.a_off_d) * M.inv_s_off;
  const double m_on = M.k_on - 0.5 * (zp * zp + za * za), m_off = M.k_off - 0.5 * (yp * yp + ya * ya);
  o.m = fmax(m_on, m_off);
  o.c_on = (float)(m_on - o.m);
  o.c_off = (float)(m_off - o.m);
  return o;
}

// obs[t, s] - m_t: <= 0 up to rounding
__device__ __forceinline__ float rel_log_obs(const Model& M, const Obs& o, int s) {
  const float fs = (float)s;
  return s == 0 ? o.c_off : fmaf(-M.half_ivar * (o.sstar - fs), (o.p - fs) + (o.p - o.sstar), o.c_on);
}

__device__ __forceinline__ float lane_value(float v, int lane) {          // lane: wave-uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// sums over the block in a fixed order, every thread receives them.  red: K * NT / 64 floats of LDS (NT = 64: unused)
template <int NT, int K>
__device__ __forceinline__ void block_sum(float (&v)[K], float* red) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum_dpp(v[k]);
  if (NT > 64) {
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
  }
}
template <int NT>
__device__ __forceinline__ float block_min(float v, float* red) {
  v = wave_min_dpp(v);
  if (NT > 64) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  }
  return v;
}

// 2^-e and e, with sum * 2^-e in [1/2, 1)
__device__ __forceinline__ float rescale(float sum, int& e) {
  e = pow2_exponent(sum);
  return ldexpf(1.0f, -e);
}

// The forward sweep of one row.  fwd (or nullptr): the rescaled forward variables, [steps, n].  -> log_prob
template <int NT>
__device__ __forceinline__ double forward_sweep(const Model& M, const float* __restrict__ pitch, const float* __restrict__ amps,
                                                int steps, float* fwd, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, n = M.n;
  float u[kQ] = {0.0f, 0.0f, 0.0f, 0.0f};
  float sum = 0.0f;
  double log_scale = 0.0;
  long long exponents = 0;
  float pc = lane < steps ? pitch[lane] : 0.0f, ac = lane < steps ? amps[lane] : 0.0f;
  for (int t0 = 0; t0 < steps; t0 += kChunk) {
    const int tn = t0 + kChunk + lane;
    const float pn = tn < steps ? pitch[tn] : 0.0f, an = tn < steps ? amps[tn] : 0.0f;      // the chunk after this one
    const int count = min(kChunk, steps - t0);
    for (int j = 0; j < count; ++j) {
      const Obs o = observe(M, lane_value(pc, j), lane_value(ac, j));
      log_scale += o.m;
      float e[kQ];
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const int s = tid + q * NT;
        e[q] = s < n ? expf(rel_log_obs(M, o, s)) : 0.0f;
      }
      float part[1] = {0.0f};
      if (t0 + j == 0) {
#pragma unroll
        for (int q = 0; q < kQ; ++q) { u[q] = e[q]; part[0] += u[q]; }
      } else {
        int ex;
        const float r = rescale(sum, ex);
        exponents += ex;
        const float base = M.other * (sum * r);
#pragma unroll
        for (int q = 0; q < kQ; ++q) { u[q] = fmaf(M.hmo, u[q] * r, base) * e[q]; part[0] += u[q]; }
      }
      if (fwd) {
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
          const int s = tid + q * NT;
          if (s < n) fwd[(size_t)(t0 + j) * n + s] = u[q];
        }
      }
      block_sum<NT, 1>(part, red);
      sum = part[0];
    }
    pc = pn; ac = an;
  }
  return log_scale + 0.6931471805599453 * (double)exponents + log((double)sum) - M.log_n;
}

template <int NT>
__global__ __launch_bounds__(NT) void log_prob_kernel(const float* __restrict__ pitch, const float* __restrict__ amps,
                                                      float* __restrict__ log_prob, int steps, Model M) {
  __shared__ float s_red[4];
  const size_t row = blockIdx.x;
  const double lp = forward_sweep<NT>(M, pitch + row * steps, amps + row * steps, steps, nullptr, s_red);
  if (threadIdx.x == 0) log_prob[row] = (float)lp;
}

template <int NT>
__global__ __launch_bounds__(NT) void log_prob_backward_kernel(const float* __restrict__ pitch, const float* __restrict__ amps,
                                                               const float* __restrict__ grad_log_prob, float* __restrict__ grad_pitch,
                                                               float* __restrict__ grad_amps, float* fwd, int steps, Model M) {
  __shared__ float s_red[12];
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, n = M.n;
  pitch += row * steps; amps += row * steps; grad_pitch += row * steps; grad_amps += row * steps;
  fwd += row * (size_t)steps * n;
  forward_sweep<NT>(M, pitch, amps, steps, fwd, s_red);
  const float gl = grad_log_prob[row];

  // the forward variables of a step are asked for three steps before they are used
  auto load_fwd = [&](int t, float (&dst)[kQ]) {
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int s = tid + q * NT;
      dst[q] = (t >= 0 && s < n) ? fwd[(size_t)t * n + s] : 0.0f;
    }
  };
  float u0[kQ], u1[kQ], u2[kQ], b[kQ];
  load_fwd(steps - 1, u0); load_fwd(steps - 2, u1); load_fwd(steps - 3, u2);
#pragma unroll
  for (int q = 0; q < kQ; ++q) b[q] = tid + q * NT < n ? 1.0f : 0.0f;

  const int last0 = ((steps - 1) / kChunk) * kChunk;
  float pc = last0 + lane < steps ? pitch[last0 + lane] : 0.0f, ac = last0 + lane < steps ? amps[last0 + lane] : 0.0f;
  for (int t0 = last0; t0 >= 0; t0 -= kChunk) {
    const int tn = t0 - kChunk + lane;
    const float pn = tn >= 0 ? pitch[tn] : 0.0f, an = tn >= 0 ? amps[tn] : 0.0f;          // the chunk before this one
    const int count = min(kChunk, steps - t0);
    for (int j = count - 1; j >= 0; --j) {
      const int t = t0 + j;
      float un[kQ];
      load_fwd(t - 3, un);
      const Obs o = observe(M, lane_value(pc, j), lane_value(ac, j));
      float w[kQ], sums[3] = {0.0f, 0.0f, 0.0f};             // sum_s w, sum_s alpha beta, sum_s alpha beta d obs / d pitch
      float prod0 = 0.0f;
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const int s = tid + q * NT;
        const float e = s < n ? expf(rel_log_obs(M, o, s)) : 0.0f;
        const float prod = u0[q] * b[q];
        const float dp = s == 0 ? (o.p - M.loc_off_p) * M.ivar_off_p : (o.p - (float)s) * M.ivar_on_p;
        if (q == 0) prod0 = prod;
        w[q] = e * b[q];
        sums[0] += w[q];
        sums[1] += prod;
        sums[2] = fmaf(prod, dp, sums[2]);
      }
      block_sum<NT, 3>(sums, s_red);
      if (tid == 0) {
        const float inv_z = 1.0f / sums[1];
        const float g0 = prod0 * inv_z;                        // gamma[t, 0]
        grad_pitch[t] = -gl * (sums[2] * inv_z);
        grad_amps[t] = -gl * ((1.0f - g0) * ((o.a - M.a_on) * M.ivar_on_a) + g0 * ((o.a - M.a_off) * M.ivar_off_a));
      }
      int ex;
      const float r = rescale(sums[0], ex);
      const float base = M.other * (sums[0] * r);
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        b[q] = tid + q * NT < n ? fmaf(M.hmo, w[q] * r, base) : 0.0f;
        u0[q] = u1[q]; u1[q] = u2[q]; u2[q] = un[q];
      }
    }
    pc = pn; ac = an;
  }
}

// max_s v[s] and the lowest s that has it, over the block
template <int NT>
__device__ __forceinline__ float best_of(const float (&v)[kQ], int n, int& arg, float* red) {
  const int tid = threadIdx.x;
  const float best = -block_min<NT>(-fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), red);
  float cand = (float)kMaxStates;
#pragma unroll
  for (int q = kQ - 1; q >= 0; --q)
    if (v[q] == best) cand = (float)(tid + q * NT);
  cand = block_min<NT>(cand, red);
  arg = cand < (float)n ? (int)cand : 0;                      // (a row of NaNs has no maximum: any state in range)
  return best;
}

template <int NT>
__global__ __launch_bounds__(NT) void viterbi_kernel(const float* __restrict__ pitch, const float* __restrict__ amps, int* __restrict__ states,
                                                     unsigned* bits, int* args, int steps, Model M) {
  __shared__ float s_red[4];
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, n = M.n;
  const int words = (steps + 31) >> 5;
  pitch += row * steps; amps += row * steps; states += row * steps;
  bits += row * (size_t)words * n; args += row * steps;

  float v[kQ];
  unsigned stayed[kQ] = {0u, 0u, 0u, 0u};
  float pc = lane < steps ? pitch[lane] : 0.0f, ac = lane < steps ? amps[lane] : 0.0f;
  for (int t0 = 0; t0 < steps; t0 += kChunk) {
    const int tn = t0 + kChunk + lane;
    const float pn = tn < steps ? pitch[tn] : 0.0f, an = tn < steps ? amps[tn] : 0.0f;
    const int count = min(kChunk, steps - t0);
    for (int j = 0; j < count; ++j) {
      const int t = t0 + j;
      const Obs o = observe(M, lane_value(pc, j), lane_value(ac, j));
      if (t == 0) {
#pragma unroll
        for (int q = 0; q < kQ; ++q) v[q] = tid + q * NT < n ? rel_log_obs(M, o, tid + q * NT) : -INFINITY;
      } else {
        int arg;
        const float best = best_of<NT>(v, n, arg, s_red);
        if (tid == 0) args[t] = arg;
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
          const int s = tid + q * NT;
          const float stay = (v[q] - best) + M.log_hold, jump = M.log_other;
          // the dense arg-max over the previous state takes the lowest index among equals
          const bool keep = stay > jump || (stay == jump && s <= arg);
          stayed[q] |= (keep ? 1u : 0u) << (t & 31);
          v[q] = s < n ? fmaxf(stay, jump) + rel_log_obs(M, o, s) : -INFINITY;
        }
      }
      if ((t & 31) == 31 || t == steps - 1) {
#pragma unroll
        for (int q = 0; q < kQ; ++q) {
          const int s = tid + q * NT;
          if (s < n) bits[(size_t)(t >> 5) * n + s] = stayed[q];
          stayed[q] = 0u;
        }
      }
    }
    pc = pn; ac = an;
  }
  int s_cur;
  best_of<NT>(v, n, s_cur, s_red);
  __syncthreads();                                             // the words and arg-maxes of the whole block are in memory

  // back trace, by the first wavefront; s_cur and t are the same in all its lanes.  Bit 0 of word 0 is never set (step 0 has
  // no transition), so the search for the step at which s_cur was entered always ends.
  if (tid >= 64) return;
  int t = steps - 1;
  while (t >= 0) {
    int entered = 0;
    for (int wd = t >> 5; wd >= 0; --wd) {
      const int top = wd == (t >> 5) ? (t & 31) : 31;
      const unsigned mask = top == 31 ? 0xffffffffu : (1u << (top + 1)) - 1u;
      const unsigned left = ~bits[(size_t)wd * n + s_cur] & mask;
      if (left) { entered = wd * 32 + 31 - __clz((int)left); break; }
    }
    for (int i = entered + lane; i <= t; i += 64) states[i] = s_cur;
    if (entered == 0) break;
    s_cur = args[entered];
    t = entered - 1;
  }
}

static int make_model(Model* m, size_t rows, int steps, int n_pitches, double hold, double other, double midi_std, double amps_on_center,
                      double amps_on_scale, double amps_off_center, double amps_off_scale) {
  if (rows == 0 || rows > (size_t)0x7fffffff || steps <= 0) return DDSP_ERR_BAD_SHAPE;
  if (!(midi_std > 0.0) || !(amps_on_scale > 0.0) || !(amps_off_scale > 0.0)) return DDSP_ERR_BAD_SHAPE;
  if (n_pitches < 2 || n_pitches > kMaxStates || !(other > 0.0) || !(hold >= other)) return DDSP_ERR_UNSUPPORTED;
  const double n = (double)n_pitches, log_2pi = 1.8378770664093453;
  m->n = n_pitches;
  m->hmo = (float)(hold - other); m->other = (float)other;
  m->log_hold = (float)log(hold); m->log_other = (float)log(other);
  m->half_ivar = (float)(0.5 / (midi_std * midi_std));
  m->ivar_on_p = (float)(1.0 / (midi_std * midi_std)); m->ivar_off_p = (float)(1.0 / (n * n));
  m->ivar_on_a = (float)(1.0 / (amps_on_scale * amps_on_scale)); m->ivar_off_a = (float)(1.0 / (amps_off_scale * amps_off_scale));
  m->loc_off_p = (float)(0.5 * n); m->a_on = (float)amps_on_center; m->a_off = (float)amps_off_center;
  m->inv_std = 1.0 / midi_std; m->inv_n = 1.0 / n; m->inv_s_on = 1.0 / amps_on_scale; m->inv_s_off = 1.0 / amps_off_scale;
  m->loc_off = 0.5 * n; m->a_on_d = amps_on_center; m->a_off_d = amps_off_center;
  m->k_on = -log(midi_std * amps_on_scale) - log_2pi;
  m->k_off = -log(n * amps_off_scale) - log_2pi;
  m->log_n = log(n);
  return DDSP_OK;
}

}  // namespace hmm
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::hmm;

#define DDSP_HMM_MODEL_PARAMS                                                                                                  \
  int n_pitches, double hold, double other, double midi_std, double amps_on_center, double amps_on_scale, double amps_off_center, \
      double amps_off_scale
#define DDSP_HMM_MODEL_ARGS n_pitches, hold, other, midi_std, amps_on_center, amps_on_scale, amps_off_center, amps_off_scale

extern "C" int ddsp_hmm_log_prob_f32(const float* pitch, const float* amps, float* log_prob, size_t rows, int steps,
                                     DDSP_HMM_MODEL_PARAMS, void* stream) {
  if (!pitch || !amps || !log_prob) return DDSP_ERR_NULL_POINTER;
  Model m;
  const int rc = make_model(&m, rows, steps, DDSP_HMM_MODEL_ARGS);
  if (rc != DDSP_OK) return rc;
  if (n_pitches <= 64 * kQ)
    hipLaunchKernelGGL(log_prob_kernel<64>, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, pitch, amps, log_prob, steps, m);
  else
    hipLaunchKernelGGL(log_prob_kernel<256>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, pitch, amps, log_prob, steps, m);
  return check_launch();
}

extern "C" size_t ddsp_hmm_log_prob_backward_workspace_bytes(int rows, int steps, int n_pitches) {
  if (rows <= 0 || steps <= 0 || n_pitches <= 0) return 0;
  return (size_t)rows * (size_t)steps * (size_t)n_pitches * sizeof(float);
}

extern "C" int ddsp_hmm_log_prob_backward_f32(const float* pitch, const float* amps, const float* grad_log_prob, float* grad_pitch,
                                              float* grad_amps, void* workspace, size_t workspace_bytes, size_t rows, int steps,
                                              DDSP_HMM_MODEL_PARAMS, void* stream) {
  if (!pitch || !amps || !grad_log_prob || !grad_pitch || !grad_amps || !workspace) return DDSP_ERR_NULL_POINTER;
  Model m;
  const int rc = make_model(&m, rows, steps, DDSP_HMM_MODEL_ARGS);
  if (rc != DDSP_OK) return rc;
  if (workspace_bytes < ddsp_hmm_log_prob_backward_workspace_bytes((int)rows, steps, n_pitches)) return DDSP_ERR_WORKSPACE;
  float* fwd = (float*)workspace;
  if (n_pitches <= 64 * kQ)
    hipLaunchKernelGGL(log_prob_backward_kernel<64>, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, pitch, amps, grad_log_prob,
                       grad_pitch, grad_amps, fwd, steps, m);
  else
    hipLaunchKernelGGL(log_prob_backward_kernel<256>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, pitch, amps,
                       grad_log_prob, grad_pitch, grad_amps, fwd, steps, m);
  return check_launch();
}

static size_t viterbi_bits_bytes(int rows, int steps, int n_pitches) {
  return (size_t)rows * (size_t)((steps + 31) / 32) * (size_t)n_pitches * sizeof(unsigned);
}

extern "C" size_t ddsp_hmm_viterbi_workspace_bytes(int rows, int steps, int n_pitches) {
  if (rows <= 0 || steps <= 0 || n_pitches <= 0) return 0;
  return viterbi_bits_bytes(rows, steps, n_pitches) + (size_t)rows * (size_t)steps * sizeof(int);
}

extern "C" int ddsp_hmm_viterbi_f32(const float* pitch, const float* amps, int* states, void* workspace, size_t workspace_bytes,
                                    size_t rows, int steps, DDSP_HMM_MODEL_PARAMS, void* stream) {
  if (!pitch || !amps || !states || !workspace) return DDSP_ERR_NULL_POINTER;
  Model m;
  const int rc = make_model(&m, rows, steps, DDSP_HMM_MODEL_ARGS);
  if (rc != DDSP_OK) return rc;
  if (workspace_bytes < ddsp_hmm_viterbi_workspace_bytes((int)rows, steps, n_pitches)) return DDSP_ERR_WORKSPACE;
  unsigned* bits = (unsigned*)workspace;
  int* args = (int*)((char*)workspace + viterbi_bits_bytes((int)rows, steps, n_pitches));
  if (n_pitches <= 64 * kQ)
    hipLaunchKernelGGL(viterbi_kernel<64>, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, pitch, amps, states, bits, args, steps, m);
  else
    hipLaunchKernelGGL(viterbi_kernel<256>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, pitch, amps, states, bits, args, steps,
                       m);
  return check_launch();
}
