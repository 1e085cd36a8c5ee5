// Host-side launch helpers: one copy for every translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "../../include/ddsp_amd.h"

namespace ddsp {

constexpr size_t kMaxDynLds = 64 * 1024;      // dynamic LDS a launch gets without asking for more (hipFuncSetAttribute)

// what an entry point returns after its launches
static inline int check_launch() { return hipGetLastError() == hipSuccess ? DDSP_OK : DDSP_ERR_LAUNCH; }

// blocks of 256 threads for n items, at least one, at most `cap` (the kernels stride over the rest)
static inline unsigned grid_for(size_t n, unsigned cap) {
  size_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// Zeroes p[0, n) with a KERNEL, for the buffers a later kernel of the same entry adds into with atomics.  hipMemsetAsync is
// captured into a graph as a memset node, and from the second replay on the runtime does not keep that node in front of the
// kernel nodes recorded behind it: the atomics land on memory that is cleared late or not yet
// (tests/test_gpu_graph_replay.py, the SpectralLoss row: the first replay has the eager bits, the next ones garbage).  A kernel
// node is ordered like every other launch of the entry.  Plain 4-byte stores, a wavefront's side by side: any alignment is
// taken, and the host emulation of csrc/general.hip (tests/hip_emu), which has no vector types, compiles this header too.
[[maybe_unused]] static __global__ void zero_f32_kernel(float* __restrict__ p, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0.0f;
}

[[maybe_unused]] static inline void zero_f32_async(float* p, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(zero_f32_kernel, dim3(grid_for(n, 8192)), dim3(256), 0, st, p, n);
}

}  // namespace ddsp
