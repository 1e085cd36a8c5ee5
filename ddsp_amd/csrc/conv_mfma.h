// What the convolution layers (dilated_conv.hip, conv2d.hip) share: a convolution as ONE matrix product on the matrix cores, its
// output [batch, positions, columns] channel-last, the K axis whatever the layer makes of its taps and source channels.
//
//   a layer's MFMA kernel (its own: conv_mfma_kernel, conv2d_mfma_kernel).  A block owns a run of 64 output positions of one batch
//                       row (a 16-row tile per wavefront) and up to 128 columns (8 column tiles, 64 accumulator registers per
//                       lane).  Per 32-deep step of K the block stages the step's weight fragments in LDS once for its four
//                       wavefronts; each lane takes its 8 activations of the step (zeros where there are none), applies ReLU and
//                       the row's power-of-two scale, splits them into fp16 hi / lo ONCE and multiplies by the staged fragments:
//                       hi hi + hi lo + lo hi as in split_f16.h.  Both loads run one step ahead, into registers, behind the matrix
//                       products of the step before; two stages in LDS, one barrier per step.  The two kernels keep a body each:
//                       as one function template over the activation load the 3 x 3 2-D layers ran 3 - 4 % slower.
//   epilogue            what both forms of both layers do to a sum: the bias, relu'(mask_src), the addend.
//   conv_absmax_kernel  the largest magnitude of W (up to 64 partials) and of act(x) per BATCH ROW (up to 16 each): what the
//                       power-of-two scales come from.  Never per call for x: a row alone gives the bits it gives inside a batch.
//   a layer's pack kernel (its own: only the layer knows how W is indexed) turns W into MFMA B fragments, fp16 hi / lo behind
//                       2^-e, once per call, and ends in split_f16.h's store_fragment.  The column tiles of one step lie side
//                       by side, a row of them per step: a block stages a run of a row.
//
// The workspace is the caller's: the exponent of W at 0, the partials of W at 256, those of the batch rows at 512, the fragments
// behind them.  No atomics, every sum in a fixed order, no host synchronisation.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "launch.h"
#include "split_f16.h"

namespace ddsp {
namespace conv_mfma {

constexpr int kWeightPartials = 64;        // at most this many blocks in the pass over W
constexpr int kRowPartials = 16;           // at most this many blocks per batch row in the pass over x
constexpr size_t kPartialItems = 4096;     // values a block of those passes takes, or more
constexpr size_t kHeaderBytes = 512;       // workspace: int exponent of W at 0, kWeightPartials floats at 256
constexpr int kTilePositions = 64;         // output positions of a block: 16 per wavefront
constexpr int kChunkTiles = 8;             // 16-column tiles of a block
constexpr int kStageLoads = kChunkTiles * 128 / 256;     // u32x4 a thread moves to stage one step's fragments
constexpr unsigned kMaxAbsmaxBlocks = 65536;

// partials[item] = max of act(v) (ReLU) or |v| over share item % per_row of row item / per_row (n values each); items in turn
[[maybe_unused]] static __global__ __launch_bounds__(256) void conv_absmax_kernel(const float* __restrict__ v, size_t n, size_t rows,
                                                                                  int per_row, int relu, float* __restrict__ partials) {
  __shared__ float lds[4];
  for (size_t item = blockIdx.x; item < rows * per_row; item += gridDim.x) {
    const float* r = v + (item / per_row) * n;
    float m = 0.0f;
    for (size_t i = (item % per_row) * 256 + threadIdx.x; i < n; i += (size_t)per_row * 256) m = fmaxf(m, relu ? r[i] : fabsf(r[i]));
    m = wave_max(m);
    __syncthreads();                                     // the previous item's reader is done
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) partials[item] = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
  }
}

// what every output element goes through after its sum
__device__ __forceinline__ float epilogue(float sum, size_t at, int col, const float* __restrict__ bias, const float* __restrict__ addend,
                                          const float* __restrict__ mask_src) {
  if (bias) sum += bias[col];
  if (mask_src) {                                        // relu'(x): 1 above 0, 0 at and below; where x is a NaN the gradient is one too
    const float m = mask_src[at];
    sum = m > 0.0f ? sum : (m != m ? m : 0.0f);
  }
  if (addend) sum += addend[at];
  return sum;
}

static inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }
// blocks a pass over n values is split into: one per kPartialItems, between 1 and `most`
static inline int partials_for(size_t n, int most) {
  const size_t p = n / kPartialItems;
  return (int)(p < 1 ? 1 : (p > (size_t)most ? (size_t)most : p));
}
// where the fragments begin: behind the header and the batch rows' partials
static inline size_t fragments_offset(int batch) { return kHeaderBytes + align256((size_t)batch * kRowPartials * sizeof(float)); }

struct Workspace {
  int* exponent;
  float* w_partials;
  float* row_partials;
  u32x4* packed;
};
static inline Workspace carve(void* workspace, int batch) {
  char* ws = static_cast<char*>(workspace);
  return {reinterpret_cast<int*>(ws), reinterpret_cast<float*>(ws + 256), reinterpret_cast<float*>(ws + kHeaderBytes),
          reinterpret_cast<u32x4*>(ws + fragments_offset(batch))};
}

// The two absmax passes, over W (n_w values) and over the batch rows of x (n_row each); how many partials each left.
struct Partials {
  int w_blocks, per_row;
};
static inline Partials launch_absmax(const Workspace& ws, const float* W, size_t n_w, const float* x, size_t n_row, int batch, int relu,
                                     hipStream_t s) {
  const Partials p = {partials_for(n_w, kWeightPartials), partials_for(n_row, kRowPartials)};
  hipLaunchKernelGGL(conv_absmax_kernel, dim3(p.w_blocks), dim3(256), 0, s, W, n_w, (size_t)1, p.w_blocks, 0, ws.w_partials);
  const size_t items = (size_t)batch * p.per_row;
  hipLaunchKernelGGL(conv_absmax_kernel, dim3((unsigned)(items < kMaxAbsmaxBlocks ? items : kMaxAbsmaxBlocks)), dim3(256), 0, s, x,
                     n_row, (size_t)batch, p.per_row, relu, ws.row_partials);
  return p;
}

}  // namespace conv_mfma
}  // namespace ddsp
