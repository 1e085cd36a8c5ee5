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

}  // namespace ddsp
