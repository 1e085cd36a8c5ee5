// The note pooling of ddsp/training/nn.py:375-557 for gfx950: get_note_mask, get_note_mask_from_onset, get_note_moments,
// pool_over_notes and get_short_note_loss_mask, forward and backward in x.
//
// The reference builds [batch, time, notes, dims] four times on the way (x * mask, the centred numerator, and the two
// time-distributed moments): 1.64 GB each at 32 x 1000 x 100 x 128.  Every mask it makes has at most one non-zero per step,
// so the work is O(batch * time * dims); here nothing larger than the mask itself exists, and a kernel's cost follows the
// mask's NON-ZEROS, which it finds with a ballot over 64 entries at a time.  The formulas hold for ANY fp32 mask (weights m
// in the mean, m^2 in the variance), not only 0 / 1.
//
//   1. note_mask_kernel      a 256-thread block per batch row.  Chunks of 256 steps: the edge of a step (pitch: q[p] != q[p-1]
//                            for p in 1 .. T-2, step 0 always, THE LAST STEP NEVER - nn.py:398-405; onset: int(onset[p]), step
//                            0 counts one) goes through an inclusive scan (64-lane __shfl_up scans, the wavefronts' totals
//                            through LDS, a carry from chunk to chunk) -> the region index.  note_on_only of get_note_mask
//                            keeps a region whose MEAN pitch is > 0, i.e. whose pitch sum is: a segmented fp64 sum rides in
//                            the same scan, the step that ends a region holds its total and is the one writer of that
//                            region's flag in LDS (no atomics).  A second walk recomputes the indices and writes the dense
//                            rows, zeros included, coalesced.
//   2. moments_kernel        a wavefront per (row, note, 256 dims).  Lanes read 64 steps of the mask column, the ballot of the
//                            non-zeros is walked in ascending time, four steps' loads in flight at once; lanes run over dims
//                            with fp64 accumulators: length = sum m, mean = sum m x / safe length, then a SECOND walk for
//                            sum (m (x - mean))^2 (the reference's two-pass form) and S2 = sum m^2 (x - mean), which the
//                            backward needs, as it needs what the fp32 mean lost (mean_lo = mean - float(mean)): x - mean
//                            cancels on a note of nearly equal values, and d std / d x is (x - mean) / (std L).  A sum-only
//                            instance is the adjoint of the spread in its values.
//   3. spread_kernel         a wavefront per (row, step, 256 dims): out[b, t, :] = sum_n m (a[b, n, :] + c[b, n, :] m (x[b, t, :]
//                            - mean[b, n, :] - mean_lo[b, n, :])), over the set bits of the mask row's ballots only.  c = NULL: the forward of
//                            pool_over_notes and (dims = 1) get_short_note_loss_mask; with c: the backward of the moments.
//
// No atomics, fixed orders of summation in time and in notes, a row's blocks see only that row: the same bits on every
// run and for any subset of the rows.  No workspace, no host synchronisation.
// Bounds (beyond them DDSP_ERR_UNSUPPORTED): max_regions <= 1024 in the mask kernel (a region's flag in LDS);
// rows * notes and rows * steps below 2^31; dims <= 256 * 65535.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "common.h"
#include "launch.h"

namespace ddsp {
namespace notes {

constexpr int kMaxRegions = 1024;
constexpr int kScan = 256;                 // steps a block scans at once (its thread count)
constexpr int kQ = 4;                      // dims a lane holds
constexpr int kDimsPerWave = 64 * kQ;
constexpr int kBatch = 4;                  // non-zero steps whose loads are in flight together
constexpr double kSafeEps = 1e-7;          // core.safe_divide's eps

__device__ __forceinline__ float lane_value(float v, int lane) {          // lane: wave-uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// ---- 1. the masks ---------------------------------------------------------------------------------------------------
// Inclusive scan over the block's 256 threads of (cnt: the edges so far; seg: the sum since the last edge, this step
// included; flag: an edge at or before this step inside the scanned range).  lds_*: 4 entries each.
__device__ __forceinline__ void block_scan(int& cnt, int& flag, double& seg, int* lds_cnt, int* lds_flag, double* lds_seg) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int c = __shfl_up(cnt, o), f = __shfl_up(flag, o);
    const double s = __shfl_up(seg, o);
    if (lane >= o) {
      cnt += c;
      if (!flag) seg += s;
      flag |= f;
    }
  }
  __syncthreads();
  if (lane == 63) { lds_cnt[wave] = cnt; lds_flag[wave] = flag; lds_seg[wave] = seg; }
  __syncthreads();
  int pc = 0, pf = 0;
  double ps = 0.0;
  for (int w = 0; w < wave; ++w) {
    pc += lds_cnt[w];
    ps = lds_flag[w] ? lds_seg[w] : ps + lds_seg[w];
    pf |= lds_flag[w];
  }
  cnt += pc;
  if (!flag) seg += ps;
  flag |= pf;
}

// does step p of the row start a region?  (p < T)
__device__ __forceinline__ int edge_at(const float* q, const float* onset, int p, int T) {
  if (p == 0) return 1;
  if (onset) return cvt_i32_saturating(onset[p]);        // truncation, as tf.cast (a NaN: 0; the counts it enters are range-checked)
  return (p < T - 1 && q[p] != q[p - 1]) ? 1 : 0;        // |diff| > 0; the last step never starts a region
}

__global__ __launch_bounds__(kScan) void note_mask_kernel(const float* __restrict__ pitch, const float* __restrict__ onset,
                                                          float* __restrict__ mask, int T, int N, FastDiv div_n, int note_on_only) {
  __shared__ int lds_cnt[5], lds_flag[5];
  __shared__ double lds_seg[5];
  __shared__ int lds_on[kMaxRegions];
  __shared__ int lds_idx[kScan];
  const int tid = threadIdx.x;
  const float* q = pitch + (size_t)blockIdx.x * (size_t)T;
  const float* on = onset ? onset + (size_t)blockIdx.x * (size_t)T : nullptr;
  float* out = mask + (size_t)blockIdx.x * (size_t)T * (size_t)N;
  const bool by_region = note_on_only && !onset;

  if (by_region) {
    for (int r = tid; r < N; r += kScan) lds_on[r] = 0;
    int carry_cnt = 0;
    double carry_seg = 0.0;
    for (int t0 = 0; t0 < T; t0 += kScan) {
      const int p = t0 + tid;
      int cnt = 0, flag = 0;
      double seg = 0.0;
      if (p < T) {
        cnt = flag = edge_at(q, nullptr, p, T);
        seg = (double)q[p];
      }
      block_scan(cnt, flag, seg, lds_cnt, lds_flag, lds_seg);
      cnt += carry_cnt;
      if (!flag) seg += carry_seg;
      if (p < T && (p == T - 1 || edge_at(q, nullptr, p + 1, T))) {      // the step that ends its region: the one writer
        const int r = cnt - 1;
        if (r < N) lds_on[r] = seg > 0.0 ? 1 : 0;
      }
      if (tid == kScan - 1) { lds_cnt[4] = cnt; lds_seg[4] = seg; }
      __syncthreads();
      carry_cnt = lds_cnt[4];
      carry_seg = lds_seg[4];
    }
  }

  int carry_cnt = 0;
  for (int t0 = 0; t0 < T; t0 += kScan) {
    const int p = t0 + tid;
    int cnt = 0, flag = 0;
    double seg = 0.0;
    if (p < T) cnt = edge_at(q, on, p, T);
    block_scan(cnt, flag, seg, lds_cnt, lds_flag, lds_seg);
    cnt += carry_cnt;
    int idx = -1;
    if (p < T && cnt >= 1 && cnt <= N) {
      idx = cnt - 1;
      if (note_on_only && !(by_region ? lds_on[idx] != 0 : q[p] > 0.0f)) idx = -1;
    }
    lds_idx[tid] = idx;
    if (tid == kScan - 1) lds_cnt[4] = cnt;
    __syncthreads();
    carry_cnt = lds_cnt[4];
    const int steps = min(kScan, T - t0);
    const unsigned total = (unsigned)steps * (unsigned)N;
    float* dst = out + (size_t)t0 * (size_t)N;
    for (unsigned j = tid; j < total; j += kScan) {
      unsigned r;
      const unsigned step = fastdiv(j, div_n, r);
      dst[j] = lds_idx[step] == (int)r ? 1.0f : 0.0f;
    }
  }
}

// ---- 2. the moments -------------------------------------------------------------------------------------------------
// Walks the non-zeros of a mask column in ascending time, kBatch at once: body(t[], m[]) gets kBatch steps and weights;
// where fewer are left the spare entries repeat the first step with weight 0.
template <class Body>
__device__ __forceinline__ void walk_column(const float* mcol, int T, int N, int lane, Body body) {
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    const float m = t < T ? mcol[(size_t)t * (size_t)N] : 0.0f;
    unsigned long long bits = __builtin_amdgcn_ballot_w64(m != 0.0f);
    while (bits) {
      int ts[kBatch];
      float ms[kBatch];
      const int first = __builtin_ctzll(bits);
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        const bool ok = bits != 0;
        const int l = ok ? __builtin_ctzll(bits) : first;
        bits &= bits - 1;
        const float v = lane_value(m, l);
        ts[k] = t0 + l;
        ms[k] = ok ? v : 0.0f;
      }
      body(ts, ms);
    }
  }
}

template <bool SUM_ONLY>
__global__ __launch_bounds__(64) void moments_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                     float* __restrict__ mean_out, float* __restrict__ std_out,
                                                     float* __restrict__ s2_out, float* __restrict__ mean_lo_out, float* __restrict__ len_out, int T,
                                                     int N, int D) {
  const int lane = threadIdx.x;
  const size_t bn = blockIdx.x, b = bn / (size_t)N, n = bn % (size_t)N;
  const int d0 = blockIdx.y * kDimsPerWave + lane;
  const float* mcol = mask + b * (size_t)T * (size_t)N + n;
  const float* xb = x + b * (size_t)T * (size_t)D;
  bool live[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) live[k] = d0 + 64 * k < D;

  double len = 0.0, acc[kQ] = {0.0, 0.0, 0.0, 0.0};
  walk_column(mcol, T, N, lane, [&](const int* ts, const float* ms) {
    float v[kBatch][kQ];
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
#pragma unroll
      for (int k = 0; k < kQ; ++k) v[j][k] = live[k] ? xb[(size_t)ts[j] * (size_t)D + (size_t)(d0 + 64 * k)] : 0.0f;
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      len += (double)ms[j];
#pragma unroll
      for (int k = 0; k < kQ; ++k) acc[k] = fma((double)ms[j], (double)v[j][k], acc[k]);
    }
  });

  float* mean_row = mean_out + bn * (size_t)D;
  if (SUM_ONLY) {
#pragma unroll
    for (int k = 0; k < kQ; ++k)
      if (live[k]) mean_row[d0 + 64 * k] = (float)acc[k];
    return;
  }
  const double safe_len = len == 0.0 ? kSafeEps : len;
  double mean[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    mean[k] = acc[k] / safe_len;
    if (live[k]) {
      mean_row[d0 + 64 * k] = (float)mean[k];
      if (mean_lo_out) mean_lo_out[bn * (size_t)D + (size_t)(d0 + 64 * k)] = (float)(mean[k] - (double)(float)mean[k]);
    }
  }
  if (len_out && blockIdx.y == 0 && lane == 0) len_out[bn] = (float)safe_len;
  if (!std_out) return;

  double num[kQ] = {0.0, 0.0, 0.0, 0.0}, s2[kQ] = {0.0, 0.0, 0.0, 0.0};
  walk_column(mcol, T, N, lane, [&](const int* ts, const float* ms) {
    float v[kBatch][kQ];
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
#pragma unroll
      for (int k = 0; k < kQ; ++k) v[j][k] = live[k] ? xb[(size_t)ts[j] * (size_t)D + (size_t)(d0 + 64 * k)] : 0.0f;
#pragma unroll
    for (int j = 0; j < kBatch; ++j)
#pragma unroll
      for (int k = 0; k < kQ; ++k) {
        const double w = (double)ms[j] * ((double)v[j][k] - mean[k]);
        num[k] = fma(w, w, num[k]);
        s2[k] = fma((double)ms[j], w, s2[k]);
      }
  });
#pragma unroll
  for (int k = 0; k < kQ; ++k)
    if (live[k]) {
      std_out[bn * (size_t)D + (size_t)(d0 + 64 * k)] = (float)sqrt(num[k] / safe_len);
      if (s2_out) s2_out[bn * (size_t)D + (size_t)(d0 + 64 * k)] = (float)s2[k];
    }
}

// ---- 3. the spread --------------------------------------------------------------------------------------------------
template <bool HAS_C>
__global__ __launch_bounds__(256) void spread_kernel(const float* __restrict__ mask, const float* __restrict__ a,
                                                     const float* __restrict__ c, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ mean_lo,
                                                     float* __restrict__ out, size_t rows_steps, int T, int N, int D) {
  const int lane = threadIdx.x & 63;
  const size_t bt = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (bt >= rows_steps) return;                                  // the whole wavefront leaves; the kernel has no barrier
  const size_t b = bt / (size_t)T;
  const int d0 = blockIdx.y * kDimsPerWave + lane;
  const float* mrow = mask + bt * (size_t)N;
  const size_t note0 = b * (size_t)N * (size_t)D;
  bool live[kQ];
  double xv[kQ], acc[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    live[k] = d0 + 64 * k < D;
    acc[k] = 0.0;
    xv[k] = (HAS_C && live[k]) ? (double)x[bt * (size_t)D + (size_t)(d0 + 64 * k)] : 0.0;
  }
  for (int n0 = 0; n0 < N; n0 += 64) {
    const int n = n0 + lane;
    const float m = n < N ? mrow[n] : 0.0f;
    unsigned long long bits = __builtin_amdgcn_ballot_w64(m != 0.0f);
    while (bits) {
      const int l = __builtin_ctzll(bits);
      bits &= bits - 1;
      const double mm = (double)lane_value(m, l);
      const size_t at = note0 + (size_t)(n0 + l) * (size_t)D;
#pragma unroll
      for (int k = 0; k < kQ; ++k)
        if (live[k]) {
          const size_t i = at + (size_t)(d0 + 64 * k);
          double v = (double)a[i];
          if (HAS_C) v = fma((double)c[i] * mm, (xv[k] - (double)mean[i]) - (mean_lo ? (double)mean_lo[i] : 0.0), v);
          acc[k] = fma(mm, v, acc[k]);
        }
    }
  }
#pragma unroll
  for (int k = 0; k < kQ; ++k)
    if (live[k]) out[bt * (size_t)D + (size_t)(d0 + 64 * k)] = (float)acc[k];
}

static inline bool below_2_31(size_t a, size_t b) { return b == 0 || a <= (size_t)0x7FFFFFFF / b; }

}  // namespace notes
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::notes;

extern "C" int ddsp_note_mask_f32(const float* pitch, const float* onset, float* mask, size_t rows, int steps, int max_regions,
                                  int note_on_only, void* stream) {
  if (!pitch || !mask) return DDSP_ERR_NULL_POINTER;
  if (steps < 2 || max_regions < 1) return DDSP_ERR_BAD_SHAPE;
  if (max_regions > kMaxRegions || !below_2_31(rows, 1)) return DDSP_ERR_UNSUPPORTED;
  if (rows == 0) return DDSP_OK;
  hipLaunchKernelGGL(note_mask_kernel, dim3((unsigned)rows), dim3(kScan), 0, (hipStream_t)stream, pitch, onset, mask, steps, max_regions,
                     make_fastdiv((uint32_t)max_regions), note_on_only ? 1 : 0);
  return check_launch();
}

extern "C" int ddsp_note_moments_f32(const float* x, const float* mask, float* mean, float* std, float* s2, float* mean_lo, float* lengths,
                                     size_t rows, int steps, int notes, int dims, int flags, void* stream) {
  if (!x || !mask || !mean) return DDSP_ERR_NULL_POINTER;
  if (steps < 1 || notes < 1 || dims < 1) return DDSP_ERR_BAD_SHAPE;
  const bool sum_only = (flags & DDSP_NOTES_SUM) != 0;
  if (sum_only && (std || s2 || mean_lo || lengths)) return DDSP_ERR_BAD_SHAPE;
  if (s2 && !std) return DDSP_ERR_BAD_SHAPE;
  const unsigned tiles = (unsigned)((dims + kDimsPerWave - 1) / kDimsPerWave);
  if (!below_2_31(rows, (size_t)notes) || !below_2_31(rows, (size_t)steps) || tiles > 65535u) return DDSP_ERR_UNSUPPORTED;
  if (rows == 0) return DDSP_OK;
  const dim3 grid((unsigned)(rows * (size_t)notes), tiles);
  if (sum_only)
    hipLaunchKernelGGL(moments_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, x, mask, mean, std, s2, mean_lo, lengths, steps, notes,
                       dims);
  else
    hipLaunchKernelGGL(moments_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, x, mask, mean, std, s2, mean_lo, lengths, steps, notes,
                       dims);
  return check_launch();
}

extern "C" int ddsp_note_spread_f32(const float* mask, const float* a, const float* c, const float* x, const float* mean,
                                    const float* mean_lo, float* out, size_t rows, int steps, int notes, int dims, void* stream) {
  if (!mask || !a || !out || (c && (!x || !mean)) || (mean_lo && !c)) return DDSP_ERR_NULL_POINTER;
  if (steps < 1 || notes < 1 || dims < 1) return DDSP_ERR_BAD_SHAPE;
  const unsigned tiles = (unsigned)((dims + kDimsPerWave - 1) / kDimsPerWave);
  if (!below_2_31(rows, (size_t)notes) || !below_2_31(rows, (size_t)steps) || tiles > 65535u) return DDSP_ERR_UNSUPPORTED;
  if (rows == 0) return DDSP_OK;
  const size_t rows_steps = rows * (size_t)steps;
  const dim3 grid((unsigned)((rows_steps + 3) / 4), tiles);
  if (c)
    hipLaunchKernelGGL(spread_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, mask, a, c, x, mean, mean_lo, out, rows_steps, steps, notes,
                       dims);
  else
    hipLaunchKernelGGL(spread_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, mask, a, c, x, mean, mean_lo, out, rows_steps, steps, notes,
                       dims);
  return check_launch();
}
