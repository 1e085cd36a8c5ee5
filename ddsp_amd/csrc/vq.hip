// ddsp/training/nn.py VectorQuantization for gfx950 (C ABI: vq_abi.h): the nearest centroid of every vector of a batch, and the
// per-centroid counts and sums the moving averages are fed with.  The reference builds an [n, k] distance matrix, an [n, k]
// one-hot matrix and a [k, n] x [n, D] product, n = rows * heads; here nothing of size [n, k] exists.
//
// x is [rows, heads * D], so vector (i, h) is row i * heads + h of the SAME memory read as [n, D]: the heads cost nothing, and
// the reference's split-and-concat copy is never made.  c [rows, heads] is indexed by that row too.
//
//   score(v, j) = |e_j|^2 / 2 - x_v . e_j        (the distance is |x_v|^2 + 2 score: the same argmin)
//
//   vq_pack_kernel     k a multiple of 16: e as MFMA B fragments, fp16 hi / lo behind ONE 2^-e (its magnitude comes from
//                      conv_mfma.h's absmax pass), once per call; D tails are zeros.  Its first k threads also leave |e_j|^2 / 2.
//   vq_mfma_kernel     a block owns 64 vectors (a 16-row tile per wavefront) and walks the codebook 128 columns at a time.  Every
//                      vector sits behind its OWN power-of-two scale, found by the four lanes that hold it: its bits never depend
//                      on its neighbours.  A step is (column chunk, 32-deep slice of D): the chunk's fragments are staged in LDS
//                      once for the four wavefronts, a lane splits its 8 values of x into fp16 hi / lo and multiplies: hi hi +
//                      hi lo + lo hi as in split_f16.h.  Both loads run a step ahead, as in the convolutions.  At a chunk's last
//                      step the accumulator tile becomes scores, and each lane carries (best score, best column) of its four rows
//                      with a strict <: columns ascend, so of equal scores the lowest stays.  At the end the sixteen lanes of a
//                      row compare (score, then column).
//   vq_plain_kernel    every other k: a block per 64 vectors, a lane each, their values in LDS; its eight wavefronts take the
//                      centroids in turns, eight at a time, dims in order with fmaf, and compare (score, then column) at the end.
//   vq_gather_kernel   z = e[c], NaN where x is not finite.
//   vq_stats_kernel    a block per (centroid, 256 dims), eight wavefronts, each over an eighth of the vectors in the reference's
//                      x_flat order (head-major).  Lanes read 512 entries of c at once; the ballots of c == j give the members,
//                      which the wavefront lists in LDS in ascending order (a lane's place is the population of the ballot below
//                      it).  Only the listed rows of x are fetched, kStatsBatch in flight at once, and added in fp64 in the
//                      list's order; the eight partial sums are added in wavefront order.  The count is the lists' length.
//                      (The first form - four wavefronts, a ballot's members fetched as soon as it was taken, so that most rows
//                      paid a latency of their own - took 245 us where this one takes 76, at 32 000 vectors and k = 512:
//                      DESIGN.md section 8.)
//
// A column's score is the same instruction sequence on the same operands wherever the column sits, so identical centroids have
// identical scores and the lower index wins.  A vector with a non-finite entry gets c = 0.
// No atomics, every sum in a fixed order, no host synchronisation, the workspace is the caller's: capturable, and the same bits
// on every run; c and z for a vector alone and inside any batch.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "../../include/ddsp_amd.h"
#include "vq_abi.h"
#include "conv_mfma.h"

namespace ddsp {
namespace vq {

using namespace conv_mfma;                   // the chunk of 8 column tiles, its staging, the absmax pass, the workspace header

constexpr int kPlainLdsDims = 128;           // dims of a vector the plain kernel keeps in LDS (beyond: read from memory)
constexpr int kPlainColumns = 8;             // centroids the plain kernel scores per pass over a vector
constexpr int kPlainWaves = 8;               // wavefronts that share a block's 64 vectors
constexpr int kStatsWaves = 8;               // wavefronts that share a centroid's vectors
constexpr int kStatsQ = 4;                   // dims a lane holds
constexpr int kStatsDims = 64 * kStatsQ;
constexpr int kStatsLoads = 8;               // 64-entry loads of c in flight together
constexpr int kStatsBatch = 8;               // member rows of x in flight together
constexpr int kStatsList = 1024;             // members a wavefront lists before it adds them

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < INFINITY; }

// |e_j|^2 / 2, dims in order: the same bits for identical rows
__device__ __forceinline__ float half_norm(const float* __restrict__ row, int D) {
  float s = 0.0f;
  for (int d = 0; d < D; ++d) s = fmaf(row[d], row[d], s);
  return 0.5f * s;
}

__global__ __launch_bounds__(256) void vq_norm_kernel(const float* __restrict__ e, float* __restrict__ half_norms, int D, int K) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < K) half_norms[j] = half_norm(e + (size_t)j * D, D);
}

// MFMA B fragments, scaled by 2^-e, as fp16 hi / lo: fragment (ks, ct) at id ks CT + ct; lane l, element q holds
// B[kk][j] = e[ct 16 + j][ks 32 + kk], kk = 8 (l / 16) + q, j = l % 16, and 0 where ks 32 + kk >= D.
__global__ __launch_bounds__(256) void vq_pack_kernel(const float* __restrict__ e, const float* __restrict__ partials, int* __restrict__ exponent,
                                                      float* __restrict__ half_norms, u32x4* __restrict__ packed, int D, int K, int n_partials) {
  const int CT = K / 16, KS = (D + 31) / 32;
  float m = 0.0f;
  for (int i = 0; i < n_partials; ++i) m = fmaxf(m, partials[i]);
  const int ex = pow2_exponent(m);
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id == 0) *exponent = ex;
  if (id < (size_t)K) half_norms[id] = half_norm(e + id * (size_t)D, D);
  const size_t frag_id = id >> 6;
  if (frag_id >= (size_t)KS * CT) return;
  const int lane = (int)(id & 63);
  const int ct = (int)(frag_id % CT), ks = (int)(frag_id / CT);
  const int col = ct * 16 + (lane & 15), d0 = ks * 32 + 8 * (lane >> 4);
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = d0 + q < D ? ldexpf(e[(size_t)col * D + d0 + q], -ex) : 0.0f;
  store_fragment(packed, frag_id, lane, v);
}

// grid: blocks of 64 vectors
__global__ __launch_bounds__(256) void vq_mfma_kernel(const float* __restrict__ x, const u32x4* __restrict__ packed,
                                                      const int* __restrict__ e_exponent, const float* __restrict__ half_norms,
                                                      int* __restrict__ c, size_t n, int D, int K) {
  __shared__ u32x4 stage[2][kChunkTiles * 128];          // the fragments of a column chunk for two steps: 32 KB
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row0 = (size_t)blockIdx.x * kTilePositions + wave * 16;
  const size_t a_row = row0 + (lane & 15);
  const int c_lane = 8 * (lane >> 4);
  const int CT = K / 16, KS = (D + 31) / 32;
  const int steps = (CT + kChunkTiles - 1) / kChunkTiles * KS;
  const float* xr = x + a_row * (size_t)D;
  // this vector's magnitude, and whether it is finite: the lanes l, l + 16, l + 32, l + 48 hold its four 8-wide slices of a step
  float m = 0.0f;
  int bad = 0;
  if (a_row < n)
    for (int d = c_lane; d < D; d += 32)
      for (int q = 0; q < 8 && d + q < D; ++q) {
        const float v = xr[d + q];
        m = fmaxf(m, fabsf(v));
        bad |= is_finite(v) ? 0 : 1;
      }
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  bad |= __shfl_xor(bad, 16);
  bad |= __shfl_xor(bad, 32);
  const int e_x = pow2_exponent(m);                      // per VECTOR
  // Step s = (column chunk s / KS, 32-deep slice s % KS).  Its fragments and this lane's 8 values of x are fetched into registers
  // one step ahead, while the matrix cores work on the step before; the fragments then go to the stage that step s - 2 used.
  u32x4 b_next[kStageLoads];
  float v_next[8];
  auto fetch = [&](int step) {
    const int ks = step % KS, ct0 = step / KS * kChunkTiles;
    const int nct = CT - ct0 < kChunkTiles ? CT - ct0 : kChunkTiles;
    const u32x4* src = packed + ((size_t)ks * CT + ct0) * 128;
#pragma unroll
    for (int i = 0; i < kStageLoads; ++i) {
      const int at = (int)threadIdx.x + 256 * i;
      if (at < nct * 128) b_next[i] = src[at];
    }
    const int d = ks * 32 + c_lane;
#pragma unroll
    for (int q = 0; q < 8; ++q) v_next[q] = 0.0f;
    if (a_row < n && d < D) {
      const float* p = xr + d;
      if (d + 8 <= D) {
        const PackedF4 p0 = *reinterpret_cast<const PackedF4*>(p), p1 = *reinterpret_cast<const PackedF4*>(p + 4);
        v_next[0] = p0.x; v_next[1] = p0.y; v_next[2] = p0.z; v_next[3] = p0.w;
        v_next[4] = p1.x; v_next[5] = p1.y; v_next[6] = p1.z; v_next[7] = p1.w;
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (d + q < D) v_next[q] = p[q];
      }
    }
  };
  // the accumulator holds rows 4 (lane / 16) + q of the tile: their scales
  int e_row[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) e_row[q] = __shfl(e_x, 4 * (lane >> 4) + q) + *e_exponent;
  float best[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  int best_col[4] = {0, 0, 0, 0};
  f32x4 acc[kChunkTiles], cross[kChunkTiles];
#pragma unroll
  for (int j = 0; j < kChunkTiles; ++j) acc[j] = cross[j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  fetch(0);
  for (int step = 0; step < steps; ++step) {
    const int ks = step % KS, ct0 = step / KS * kChunkTiles;
    const int nct = CT - ct0 < kChunkTiles ? CT - ct0 : kChunkTiles;
    u32x4* buf = stage[step & 1];                        // its readers of step - 2 are behind the barrier of step - 1
#pragma unroll
    for (int i = 0; i < kStageLoads; ++i) {
      const int at = (int)threadIdx.x + 256 * i;
      if (at < nct * 128) buf[at] = b_next[i];
    }
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = ldexpf(v_next[q], -e_x);
    f16x8 a_hi, a_lo;
    split8(v, a_hi, a_lo);
    __syncthreads();
    if (step + 1 < steps) fetch(step + 1);
#pragma unroll
    for (int j = 0; j < kChunkTiles; ++j) {
      if (j < nct) {                                     // block-uniform
        const f16x8 b_hi = __builtin_bit_cast(f16x8, buf[j * 128 + lane]), b_lo = __builtin_bit_cast(f16x8, buf[j * 128 + 64 + lane]);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_hi, acc[j], 0, 0, 0);
        cross[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, b_lo, cross[j], 0, 0, 0);
        cross[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, b_hi, cross[j], 0, 0, 0);
      }
    }
    if (ks + 1 < KS) continue;
    // the chunk's products are complete: scores, and the running argmin over ascending columns
#pragma unroll
    for (int j = 0; j < kChunkTiles; ++j) {
      if (j < nct) {
        const int col = (ct0 + j) * 16 + (lane & 15);
        const float hn = half_norms[col];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float score = hn - ldexpf(combine(acc[j][q], cross[j][q]), e_row[q]);
          if (score < best[q]) {
            best[q] = score;
            best_col[q] = col;
          }
        }
        acc[j] = cross[j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
  }
  // across the sixteen lanes of a row: the lower score, of equal scores the lower column
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float s = __shfl_xor(best[q], o);
      const int col = __shfl_xor(best_col[q], o);
      if (s < best[q] || (s == best[q] && col < best_col[q])) {
        best[q] = s;
        best_col[q] = col;
      }
    }
    const int row_bad = __shfl(bad, 4 * (lane >> 4) + q);
    const size_t row = row0 + 4 * (lane >> 4) + q;
    if ((lane & 15) == 0 && row < n) c[row] = row_bad ? 0 : best_col[q];
  }
}

// grid: blocks of 64 vectors, a lane each; the block's wavefronts share the centroids, kPlainColumns at a time in turns
__global__ __launch_bounds__(64 * kPlainWaves) void vq_plain_kernel(const float* __restrict__ x, const float* __restrict__ e,
                                                                    const float* __restrict__ half_norms, int* __restrict__ c, size_t n, int D,
                                                                    int K) {
  extern __shared__ float lds[];                         // the wavefronts' (best score, best column), then x as [d][lane] if D <= kPlainLdsDims
  float* wave_best = lds;
  int* wave_col = reinterpret_cast<int*>(lds + 64 * kPlainWaves);
  float* tile = lds + 128 * kPlainWaves;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t row = (size_t)blockIdx.x * 64 + lane;
  const bool live = row < n;
  const float* xr = x + (live ? row : 0) * (size_t)D;
  const bool staged = D <= kPlainLdsDims;
  if (staged) {
    for (int d = wave; d < D; d += kPlainWaves) tile[d * 64 + lane] = xr[d];
    __syncthreads();
  }
  float best = INFINITY;
  int best_col = 0;
  for (int j0 = wave * kPlainColumns; j0 < K; j0 += kPlainWaves * kPlainColumns) {
    const float* er[kPlainColumns];
    float dot[kPlainColumns];
#pragma unroll
    for (int u = 0; u < kPlainColumns; ++u) {
      er[u] = e + (size_t)(j0 + u < K ? j0 + u : K - 1) * D;      // past the end: the last one again, ignored below
      dot[u] = 0.0f;
    }
#pragma unroll 4
    for (int d = 0; d < D; ++d) {
      const float v = staged ? tile[d * 64 + lane] : xr[d];
#pragma unroll
      for (int u = 0; u < kPlainColumns; ++u) dot[u] = fmaf(v, er[u][d], dot[u]);      // wave-uniform addresses: scalar loads
    }
#pragma unroll
    for (int u = 0; u < kPlainColumns; ++u) {
      const float score = half_norms[j0 + u < K ? j0 + u : K - 1] - dot[u];
      if (j0 + u < K && score < best) {
        best = score;
        best_col = j0 + u;
      }
    }
  }
  wave_best[wave * 64 + lane] = best;
  wave_col[wave * 64 + lane] = best_col;
  __syncthreads();
  if (wave != 0) return;
  // the wavefronts took the columns in turns: the lower score, of equal scores the lower column
  for (int w = 1; w < kPlainWaves; ++w) {
    const float s = wave_best[w * 64 + lane];
    const int col = wave_col[w * 64 + lane];
    if (s < best || (s == best && col < best_col)) {
      best = s;
      best_col = col;
    }
  }
  bool bad = false;
  for (int d = 0; d < D; ++d) bad = bad || !is_finite(staged ? tile[d * 64 + lane] : xr[d]);
  if (live) c[row] = bad ? 0 : best_col;
}

__global__ __launch_bounds__(256) void vq_gather_kernel(const float* __restrict__ x, const float* __restrict__ e, const int* __restrict__ c,
                                                        float* __restrict__ z, size_t total, int D) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t at = (size_t)blockIdx.x * 256 + threadIdx.x; at < total; at += stride) {
    const size_t row = at / (size_t)D;
    const int d = (int)(at - row * (size_t)D);
    z[at] = is_finite(x[at]) ? e[(size_t)c[row] * D + d] : NAN;
  }
}

// grid (k, dims / 256); wavefront w takes the x_flat rows [w segment, (w + 1) segment), x_flat row m = h rows + i
__global__ __launch_bounds__(64 * kStatsWaves) void vq_stats_kernel(const float* __restrict__ x, const int* __restrict__ c,
                                                                    float* __restrict__ counts, float* __restrict__ sums, FastDiv div_rows,
                                                                    uint32_t n, uint32_t segment, int heads, int D) {
  __shared__ double part[kStatsWaves][kStatsDims];
  __shared__ long long part_count[kStatsWaves];
  __shared__ uint32_t member_list[kStatsWaves][kStatsList];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x;
  const int d0 = blockIdx.y * kStatsDims + lane;
  bool live[kStatsQ];
#pragma unroll
  for (int k = 0; k < kStatsQ; ++k) live[k] = d0 + 64 * k < D;
  double acc[kStatsQ] = {0.0, 0.0, 0.0, 0.0};
  long long count = 0;
  uint32_t* members = member_list[wave];
  int fill = 0;                                          // wave-uniform
  // adds the listed rows of x, kStatsBatch in flight at once, in the order of the list
  auto drain = [&]() {
    DDSP_WAVE_LDS_SYNC();                                // the list is this wavefront's own
    for (int p = 0; p < fill; p += kStatsBatch) {
      size_t at[kStatsBatch];
      bool ok[kStatsBatch];
#pragma unroll
      for (int b = 0; b < kStatsBatch; ++b) {
        ok[b] = p + b < fill;
        uint32_t i;
        const uint32_t h = fastdiv(members[ok[b] ? p + b : p], div_rows, i);
        at[b] = ((size_t)i * heads + h) * (size_t)D;
      }
      float v[kStatsBatch][kStatsQ];
#pragma unroll
      for (int b = 0; b < kStatsBatch; ++b)
#pragma unroll
        for (int k = 0; k < kStatsQ; ++k) v[b][k] = live[k] ? x[at[b] + (size_t)(d0 + 64 * k)] : 0.0f;
#pragma unroll
      for (int b = 0; b < kStatsBatch; ++b)
#pragma unroll
        for (int k = 0; k < kStatsQ; ++k) acc[k] += ok[b] ? (double)v[b][k] : 0.0;
    }
    DDSP_WAVE_LDS_SYNC();                                // read before the next scan overwrites it
    count += fill;
    fill = 0;
  };
  const uint32_t begin = (uint32_t)wave * segment;
  const uint32_t end = begin + segment < n ? begin + segment : n;        // kStatsWaves segment < 2^32
  for (uint32_t m0 = begin; m0 < end; m0 += 64 * kStatsLoads) {
    int member[kStatsLoads];
#pragma unroll
    for (int q = 0; q < kStatsLoads; ++q) {
      const uint32_t m = m0 + 64 * q + lane;
      uint32_t i;
      const uint32_t h = fastdiv(m < end ? m : begin, div_rows, i);
      member[q] = m < end && c[(size_t)i * heads + h] == j;
    }
#pragma unroll
    for (int q = 0; q < kStatsLoads; ++q) {
      const unsigned long long bits = __builtin_amdgcn_ballot_w64(member[q] != 0);
      if (member[q]) members[fill + __builtin_popcountll(bits & ((1ull << lane) - 1ull))] = m0 + 64 * q + lane;
      fill += __builtin_popcountll(bits);
    }
    if (fill > kStatsList - 64 * kStatsLoads) drain();   // the next scan may find this many
  }
  drain();
#pragma unroll
  for (int k = 0; k < kStatsQ; ++k) part[wave][lane + 64 * k] = acc[k];
  if (lane == 0) part_count[wave] = count;
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int k = 0; k < kStatsQ; ++k) {
    double s = part[0][lane + 64 * k];
    for (int w = 1; w < kStatsWaves; ++w) s += part[w][lane + 64 * k];
    if (live[k]) sums[(size_t)j * D + (size_t)(d0 + 64 * k)] = (float)s;
  }
  if (blockIdx.y == 0 && lane == 0) {
    long long total = 0;
    for (int w = 0; w < kStatsWaves; ++w) total += part_count[w];
    counts[j] = (float)total;
  }
}

static inline bool well_formed(int rows, int heads, int k, int dims) { return rows >= 0 && heads >= 1 && k >= 1 && dims >= 1; }
static inline bool supported(int rows, int heads, int k, int dims) {
  return k <= DDSP_VQ_MAX_CENTROIDS && dims <= DDSP_VQ_MAX_DIMS && (long long)rows * heads <= (long long)INT_MAX;
}
static inline size_t norms_bytes(int k) { return align256((size_t)k * sizeof(float)); }
static inline size_t packed_bytes(int k, int dims) { return k % 16 ? 0 : (size_t)((dims + 31) / 32) * (k / 16) * 128 * sizeof(u32x4); }

}  // namespace vq
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::vq;

// the exponent of e at 0, the partials of its magnitude at 256, |e_j|^2 / 2 at 512, the fragments behind them
extern "C" size_t ddsp_vq_workspace_bytes(int k, int dims) {
  if (!well_formed(0, 1, k, dims) || !supported(0, 1, k, dims)) return 0;
  return kHeaderBytes + norms_bytes(k) + packed_bytes(k, dims);
}

extern "C" int ddsp_vq_assign_f32(const float* x, const float* e, int* c, float* z, void* workspace, size_t workspace_bytes, int rows, int heads,
                                  int k, int dims, void* stream) {
  if (!x || !e || !c || !z) return DDSP_ERR_NULL_POINTER;
  if (!well_formed(rows, heads, k, dims)) return DDSP_ERR_BAD_SHAPE;
  if (!supported(rows, heads, k, dims)) return DDSP_ERR_UNSUPPORTED;
  if (rows == 0) return DDSP_OK;
  if (!workspace) return DDSP_ERR_NULL_POINTER;
  if (workspace_bytes < ddsp_vq_workspace_bytes(k, dims)) return DDSP_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  int* exponent = reinterpret_cast<int*>(ws);
  float* partials = reinterpret_cast<float*>(ws + 256);
  float* half_norms = reinterpret_cast<float*>(ws + kHeaderBytes);
  u32x4* packed = reinterpret_cast<u32x4*>(ws + kHeaderBytes + norms_bytes(k));
  const size_t n = (size_t)rows * heads;
  if (k % 16 == 0) {
    const size_t n_e = (size_t)k * dims;
    const int blocks = partials_for(n_e, kWeightPartials);
    hipLaunchKernelGGL(conv_absmax_kernel, dim3(blocks), dim3(256), 0, s, e, n_e, (size_t)1, blocks, 0, partials);
    const size_t pack_threads = (size_t)((dims + 31) / 32) * (k / 16) * 64;
    hipLaunchKernelGGL(vq_pack_kernel, dim3((unsigned)((pack_threads + 255) / 256)), dim3(256), 0, s, e, partials, exponent, half_norms, packed, dims,
                       k, blocks);
    hipLaunchKernelGGL(vq_mfma_kernel, dim3((unsigned)((n + kTilePositions - 1) / kTilePositions)), dim3(256), 0, s, x, packed, exponent, half_norms,
                       c, n, dims, k);
  } else {
    hipLaunchKernelGGL(vq_norm_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, s, e, half_norms, dims, k);
    const size_t lds = (128 * kPlainWaves + (dims <= kPlainLdsDims ? (size_t)dims * 64 : 0)) * sizeof(float);
    hipLaunchKernelGGL(vq_plain_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64 * kPlainWaves), lds, s, x, e, half_norms, c, n, dims, k);
  }
  const size_t total = n * (size_t)dims;
  hipLaunchKernelGGL(vq_gather_kernel, dim3(grid_for(total, 65536)), dim3(256), 0, s, x, e, c, z, total, dims);
  return check_launch();
}

extern "C" int ddsp_vq_statistics_f32(const float* x, const int* c, float* counts, float* sums, int rows, int heads, int k, int dims,
                                      void* stream) {
  if (!counts || !sums || (rows > 0 && (!x || !c))) return DDSP_ERR_NULL_POINTER;
  if (!well_formed(rows, heads, k, dims)) return DDSP_ERR_BAD_SHAPE;
  if (!supported(rows, heads, k, dims)) return DDSP_ERR_UNSUPPORTED;
  const size_t n = (size_t)rows * heads;
  const size_t span = 64 * kStatsLoads;
  const size_t segment = ((n + kStatsWaves - 1) / kStatsWaves + span - 1) / span * span;
  const dim3 grid((unsigned)k, (unsigned)((dims + kStatsDims - 1) / kStatsDims));
  hipLaunchKernelGGL(vq_stats_kernel, grid, dim3(64 * kStatsWaves), 0, (hipStream_t)stream, x, c, counts, sums,
                     make_fastdiv((uint32_t)(rows > 0 ? rows : 1)), (uint32_t)n, (uint32_t)segment, heads, dims);
  return check_launch();
}
