// losses.wasserstein_distance (ddsp/losses.py:632-686; WassersteinConsistencyLoss, :584-629, is its mean in MIDI) for gfx950,
// forward and backward.
//
// The reference sorts both sides and their concatenation, finds each merged value's place in either side with searchsorted
// and gathers the cumulated weights: a dozen ops over [rows, n_u + n_v] arrays.  Per row that is a few hundred floats, so a
// block of 256 threads owns one row and everything stays in LDS, as in consistency.hip:
//
//   1. stage   key_e = (hi, lo) of the value of element e of the concatenation [u, v] - in MIDI mode hz_to_midi(Hz) as the
//              fp64-derived fp32 pair, so that a difference of two keys is good to an ulp of the DIFFERENCE; the order is that of
//              the MIDI values (hz_to_midi(f <= 0) = 0 sits above 0 < f < 8.18 Hz).  A NaN among the row's values or weights is
//              found here (a block-wide sum of flags): the row's distance, and every gradient of the row, is NaN.
//   2. rank    thread tid owns the elements tid + 256 q.  rank_e = the number of elements whose (hi, lo, position) is smaller:
//              stable (u before v, a lower index first), no barrier, deterministic.  The other keys are read from LDS two at a
//              time as 16-byte broadcasts.  QUADRATIC: n compares per element - 200 per thread at 100 + 100 sinusoids, 16 k
//              at the bound of 1024 + 1024.  A documented limit, not a tuned path.
//   3. scatter key, u-weight-or-0 and v-weight-or-0 to slot rank_e (weights None: 1, divided by n_side at the end, as the
//              reference's index / float(n)).  The owner keeps rank_e in a register, so no source index is stored.
//   4. scan    U_r, V_r = inclusive sums of the two weight columns over the sorted order, kept apart and subtracted at the end
//              as the reference does: thread t walks the contiguous chunk t serially, the chunk totals are scanned over the
//              wavefront by shuffles and over the four wavefronts through LDS - one fixed order, in fp64.  Values tied within
//              or across the sides have delta = 0 between them, so the inclusive sum over the stable order equals the
//              reference's searchsorted(side='right') wherever it is multiplied by something.
//   5. reduce  W = (sum_r delta_r |D_r|^p)^(1/p), D = U - V, delta_r = key_{r+1} - key_r: fp64 partials in a fixed order.
//   6. backward recomputes 1-4 (nothing is stored), then scans c_r = delta_r d|D_r|^p/dD_r from the far end (the same scan,
//              the chunks taken in reverse): S_r = sum_{r' >= r} c_r'.  With r = rank_e:
//                  dW/du_weight_e = S_r, dW/dv_weight_e = -S_r, dW/dvalue_e = |D_{r-1}|^p - |D_r|^p
//              (the first term absent at r = 0, the second at r = n - 1), all times 1 / (2 W) for p = 2; in MIDI mode times
//              12 / ln 2 / f, and 0 for f <= 0.  The owner of e writes them: no atomics, every element written exactly once.
//
// The weights are NOT normalised: the reference calls safe_divide(u_cdf, ...) and drops the result (losses.py:673, 683).
//
// Bounds (beyond them DDSP_ERR_UNSUPPORTED): n_u, n_v <= 1024 each; p = 1 or 2 (compiled instances).
// LDS: 3 arrays of 2048 x 8 bytes (keys, later S; sorted keys; sorted weights, later D) + 12 doubles = 49,248 bytes, static:
// three blocks per CU.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "common.h"
#include "consistency_common.h"
#include "launch.h"

namespace ddsp {
namespace wasserstein {

using consistency::block_sum;
using consistency::hz_to_midi;
using consistency::kMidiSlope;
using consistency::kThreads;
using consistency::kWaves;

constexpr int kMaxSide = 1024;
constexpr int kMaxN = 2 * kMaxSide;
constexpr int kOwn = kMaxN / kThreads;      // elements a thread owns: e = tid + 256 q

struct alignas(8) Key { float hi, lo; };
union alignas(8) KeyOrSum { Key key; double S; };          // the staged keys; after the ranking, S_r of the backward pass
union alignas(8) WeightsOrD { float w[2]; double D; };      // sorted {u weight, v weight}; after the scan, D_r = U_r - V_r

// inclusive scan of (a, b) over the block's threads in thread order.  sa, sb: kWaves doubles of LDS each.
__device__ __forceinline__ void block_scan2(double& a, double& b, double* sa, double* sb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double pa = __shfl_up(a, o), pb = __shfl_up(b, o);
    if (lane >= o) { a += pa; b += pb; }
  }
  __syncthreads();
  if (lane == 63) { sa[wave] = a; sb[wave] = b; }
  __syncthreads();
  double oa = 0.0, ob = 0.0;
#pragma unroll
  for (int w = 0; w < kWaves - 1; ++w)
    if (w < wave) { oa += sa[w]; ob += sb[w]; }
  a += oa;
  b += ob;
}

// key_{r+1} - key_r of the sorted keys, good to an ulp of the difference
__device__ __forceinline__ float delta_at(const Key* val, int r) {
  return (val[r + 1].hi - val[r].hi) + (val[r + 1].lo - val[r].lo);
}

template <int P> __device__ __forceinline__ double pow_abs(double d) { return P == 1 ? fabs(d) : d * d; }
// d |D|^p / dD: sign(D) with sign(0) = 0, or 2 D
template <int P> __device__ __forceinline__ double dpow_abs(double d) {
  return P == 1 ? (double)((d > 0.0) - (d < 0.0)) : 2.0 * d;
}

static_assert(sizeof(KeyOrSum) == 8 && sizeof(WeightsOrD) == 8 && sizeof(Key) == 8, "8 bytes per element and array");

struct Args { int n_u, n_v, midi; };

template <int P, bool BWD>
__global__ __launch_bounds__(kThreads) void wasserstein_kernel(const float* __restrict__ u_values, const float* __restrict__ v_values,
                                                               const float* __restrict__ u_weights, const float* __restrict__ v_weights,
                                                               float* __restrict__ distance, const float* __restrict__ g_distance,
                                                               float* __restrict__ g_u_values, float* __restrict__ g_v_values,
                                                               float* __restrict__ g_u_weights, float* __restrict__ g_v_weights, Args p) {
  __shared__ __attribute__((aligned(16))) KeyOrSum s_key[kMaxN];     // read as float4: two keys at a time
  __shared__ Key s_val[kMaxN];
  __shared__ WeightsOrD s_w[kMaxN];
  __shared__ double s_red[kWaves], s_sa[kWaves], s_sb[kWaves];
  const size_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const int n_u = p.n_u, n_v = p.n_v, n = n_u + n_v;
  u_values += row * n_u; v_values += row * n_v;
  if (u_weights) u_weights += row * n_u;
  if (v_weights) v_weights += row * n_v;

  // ---- 1. stage --------------------------------------------------------------------------------------------------------------
  float raw[kOwn], wgt[kOwn];
  bool bad = false;
#pragma unroll
  for (int q = 0; q < kOwn; ++q) {
    const int e = tid + q * kThreads;
    raw[q] = 0.0f; wgt[q] = 1.0f;
    if (e < n) {
      const bool is_u = e < n_u;
      const float* wp = is_u ? u_weights : v_weights;
      const int j = is_u ? e : e - n_u;
      raw[q] = is_u ? u_values[j] : v_values[j];
      if (wp) wgt[q] = wp[j];
      Key k;
      if (p.midi) k.hi = hz_to_midi(raw[q], k.lo);
      else { k.hi = raw[q]; k.lo = 0.0f; }
      if (!(fabsf(k.hi) < INFINITY)) k.lo = 0.0f;       // an infinite value: ordered by position among its like
      bad = bad || raw[q] != raw[q] || wgt[q] != wgt[q];
      s_key[e].key = k;
    }
  }
  if (tid == 0 && (n & 1)) s_key[n].key = Key{INFINITY, 0.0f};     // the pair read of an odd row: never smaller than anything
  const bool nan_row = block_sum(bad ? 1.0 : 0.0, s_red) > 0.0;    // (its barriers also publish the keys)
  if (nan_row) {
    const float qnan = __builtin_nanf("");
    if (!BWD) {
      if (tid == 0) distance[row] = qnan;
    } else {
      for (int e = tid; e < n; e += kThreads) {
        const bool is_u = e < n_u;
        const size_t at = is_u ? row * n_u + e : row * n_v + (e - n_u);
        (is_u ? g_u_values : g_v_values)[at] = qnan;
        float* gw = is_u ? g_u_weights : g_v_weights;
        if (gw) gw[at] = qnan;
      }
    }
    return;
  }

  // ---- 2. rank by counting, 3. scatter ------------------------------------------------------------------------------------------
  int rank[kOwn];
  const float4* pairs = reinterpret_cast<const float4*>(s_key);
  const int n_pairs = (n + 1) >> 1;
#pragma unroll
  for (int q = 0; q < kOwn; ++q) {
    const int e = tid + q * kThreads;
    rank[q] = 0;
    if (e < n) {
      const Key me = s_key[e].key;
      int cnt = 0;
      for (int jp = 0; jp < n_pairs; ++jp) {
        const float4 o = pairs[jp];                     // keys 2 jp and 2 jp + 1: the same address in every lane
        const int j = 2 * jp;
        cnt += (o.x < me.hi) || (o.x == me.hi && (o.y < me.lo || (o.y == me.lo && j < e)));
        cnt += (o.z < me.hi) || (o.z == me.hi && (o.w < me.lo || (o.w == me.lo && j + 1 < e)));
      }
      rank[q] = cnt;                                    // < n: an element is never smaller than itself
      const bool is_u = e < n_u;
      s_val[cnt] = me;
      s_w[cnt].w[0] = is_u ? wgt[q] : 0.0f;
      s_w[cnt].w[1] = is_u ? 0.0f : wgt[q];
    }
  }
  __syncthreads();

  // ---- 4. scan, 5. reduce ---------------------------------------------------------------------------------------------------------
  const int chunk = (n + kThreads - 1) / kThreads;
  const double den_u = u_weights ? 1.0 : (double)n_u, den_v = v_weights ? 1.0 : (double)n_v;
  double sum = 0.0;
  {
    const int lo = min(tid * chunk, n), hi = min(lo + chunk, n);
    double U = 0.0, V = 0.0;
    for (int r = lo; r < hi; ++r) { U += (double)s_w[r].w[0]; V += (double)s_w[r].w[1]; }
    const double own_u = U, own_v = V;
    block_scan2(U, V, s_sa, s_sb);
    U -= own_u; V -= own_v;                             // what lies before this chunk
    for (int r = lo; r < hi; ++r) {
      U += (double)s_w[r].w[0]; V += (double)s_w[r].w[1];
      const double D = U / den_u - V / den_v;
      s_w[r].D = D;
      if (r < n - 1) sum += (double)delta_at(s_val, r) * pow_abs<P>(D);
    }
  }
  const double Q = block_sum(sum, s_red);               // (its barriers also publish D)
  const double W = P == 1 ? Q : sqrt(Q);
  if (!BWD) {
    if (tid == 0) distance[row] = (float)W;
    return;
  }

  // ---- 6. backward ------------------------------------------------------------------------------------------------------------------
  {
    const int c = kThreads - 1 - tid;                   // the chunks in reverse: the scan over threads sums what lies beyond
    const int lo = min(c * chunk, n), hi = min(lo + chunk, n);
    double S = 0.0, none = 0.0;
    for (int r = lo; r < hi; ++r)
      if (r < n - 1) S += (double)delta_at(s_val, r) * dpow_abs<P>(s_w[r].D);
    const double own = S;
    block_scan2(S, none, s_sa, s_sb);
    S -= own;                                           // what lies beyond this chunk
    for (int r = hi - 1; r >= lo; --r) {
      if (r < n - 1) S += (double)delta_at(s_val, r) * dpow_abs<P>(s_w[r].D);
      s_key[r].S = S;
    }
  }
  __syncthreads();
  const double coef = (double)g_distance[row] * (P == 1 ? 1.0 : 1.0 / (2.0 * W));
#pragma unroll
  for (int q = 0; q < kOwn; ++q) {
    const int e = tid + q * kThreads;
    if (e < n) {
      const int r = rank[q];
      const bool is_u = e < n_u;
      const size_t at = is_u ? row * n_u + e : row * n_v + (e - n_u);
      double gv = (r > 0 ? pow_abs<P>(s_w[r - 1].D) : 0.0) - (r < n - 1 ? pow_abs<P>(s_w[r].D) : 0.0);
      gv *= coef;
      if (p.midi) gv = raw[q] > 0.0f ? gv * (double)kMidiSlope / (double)raw[q] : 0.0;
      (is_u ? g_u_values : g_v_values)[at] = (float)gv;
      float* gw = is_u ? g_u_weights : g_v_weights;
      if (gw) gw[at] = (float)(is_u ? coef * s_key[r].S : -coef * s_key[r].S);
    }
  }
}

static int check_args(Args* a, size_t rows, int n_u, int n_v, int p, int flags) {
  if (rows == 0 || rows > (size_t)0x7fffffff || n_u <= 0 || n_v <= 0) return DDSP_ERR_BAD_SHAPE;
  if (n_u > kMaxSide || n_v > kMaxSide || (p != 1 && p != 2) || (flags & ~DDSP_WASSERSTEIN_MIDI)) return DDSP_ERR_UNSUPPORTED;
  a->n_u = n_u; a->n_v = n_v; a->midi = (flags & DDSP_WASSERSTEIN_MIDI) ? 1 : 0;
  return DDSP_OK;
}

template <int P, bool BWD>
static int launch(const float* u_values, const float* v_values, const float* u_weights, const float* v_weights, float* distance,
                  const float* g_distance, float* g_u_values, float* g_v_values, float* g_u_weights, float* g_v_weights, size_t rows,
                  const Args& a, void* stream) {
  hipLaunchKernelGGL((wasserstein_kernel<P, BWD>), dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, u_values, v_values,
                     u_weights, v_weights, distance, g_distance, g_u_values, g_v_values, g_u_weights, g_v_weights, a);
  return check_launch();
}

}  // namespace wasserstein
}  // namespace ddsp

using namespace ddsp::wasserstein;

extern "C" int ddsp_wasserstein_f32(const float* u_values, const float* v_values, const float* u_weights, const float* v_weights,
                                    float* distance, size_t rows, int n_u, int n_v, int p, int flags, void* stream) {
  if (!u_values || !v_values || !distance) return DDSP_ERR_NULL_POINTER;
  Args a;
  const int rc = check_args(&a, rows, n_u, n_v, p, flags);
  if (rc != DDSP_OK) return rc;
  if (p == 1)
    return launch<1, false>(u_values, v_values, u_weights, v_weights, distance, nullptr, nullptr, nullptr, nullptr, nullptr, rows, a, stream);
  return launch<2, false>(u_values, v_values, u_weights, v_weights, distance, nullptr, nullptr, nullptr, nullptr, nullptr, rows, a, stream);
}

extern "C" int ddsp_wasserstein_backward_f32(const float* u_values, const float* v_values, const float* u_weights,
                                             const float* v_weights, const float* grad_distance, float* grad_u_values,
                                             float* grad_v_values, float* grad_u_weights, float* grad_v_weights, size_t rows, int n_u,
                                             int n_v, int p, int flags, void* stream) {
  if (!u_values || !v_values || !grad_distance || !grad_u_values || !grad_v_values) return DDSP_ERR_NULL_POINTER;
  if ((u_weights == nullptr) != (grad_u_weights == nullptr) || (v_weights == nullptr) != (grad_v_weights == nullptr))
    return DDSP_ERR_NULL_POINTER;
  Args a;
  const int rc = check_args(&a, rows, n_u, n_v, p, flags);
  if (rc != DDSP_OK) return rc;
  if (p == 1)
    return launch<1, true>(u_values, v_values, u_weights, v_weights, nullptr, grad_distance, grad_u_values, grad_v_values, grad_u_weights,
                           grad_v_weights, rows, a, stream);
  return launch<2, true>(u_values, v_values, u_weights, v_weights, nullptr, grad_distance, grad_u_values, grad_v_values, grad_u_weights,
                         grad_v_weights, rows, a, stream);
}
