// The split-fp16 operand of the matrix-core kernels: x = hi + lo / 2048, hi and lo two fp16 numbers - 22 bits of x while x is
// inside fp16's normal range (common.h's pow2_exponent brings data of any scale there first).  A product of two such operands
// is three MFMAs, hi hi into `acc` and hi lo + lo hi into `cross`, put together by combine().  The parity tolerances rest on
// this contract, so it is stated here once; the kernels keep only what is theirs (layouts, and forms of the split that are
// not this one: harmonic_table.hip's wt_rest_halves).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddsp {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));      // an MFMA A / B fragment of v_mfma_f32_16x16x32_f16
typedef float f32x4 __attribute__((ext_vector_type(4)));         // its accumulator; four consecutive VGPRs
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));      // (an array of HIP's uint4 - a struct of unions - stays in scratch)
typedef __fp16 h16x2 __attribute__((ext_vector_type(2)));        // what v_cvt_pkrtz_f16_f32 returns

constexpr float kLoScale = 2048.0f;

// 16 bytes from a 4-byte aligned address
struct __attribute__((packed, aligned(4))) PackedF4 { float x, y, z, w; };
struct __attribute__((packed, aligned(4))) PackedU4 { uint32_t x, y, z, w; };

__device__ __forceinline__ void split(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)((v - (float)hi) * kLoScale);
}
// The same 22 bits cut so that BOTH parts sit on one scale: s v = hi + lo, s a power of two that brings the data near the top of
// fp16's range (the caller's to choose, and to bound: s |v| must stay below 65504).  hi hi, hi lo and lo hi then add up in ONE
// fp32 accumulator and the product is acc / (s_a s_b) - noise_mfma65_kernel's FIR, whose accumulator moves between k-steps.
// lo is at most half a unit of hi's last place: below s |v| = 2^-3 it is an fp16 subnormal (below 2^-25: zero).  gfx950's matrix
// cores take subnormal inputs as they are: tests/test_gpu_noise_single_accumulator.py holds the kernel to a bound that operands
// with flushed lo parts miss ninefold.
__device__ __forceinline__ void split_scaled(float v, float s, _Float16& hi, _Float16& lo) {
  const float t = v * s;
  hi = (_Float16)t;
  lo = (_Float16)(t - (float)hi);
}
__device__ __forceinline__ void split8(const float (&v)[8], f16x8& hi, f16x8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    _Float16 h, l;
    split(v[e], h, l);
    hi[e] = h;
    lo[e] = l;
  }
}
// How a pack kernel ends: this lane's 8 values of B fragment `frag_id`, already behind the scale, split and stored where the
// multiplying kernels read them - part hi at u32x4 index frag_id 128 + lane, part lo 64 further.
__device__ __forceinline__ void store_fragment(u32x4* packed, size_t frag_id, int lane, const float (&v)[8]) {
  f16x8 hi, lo;
  split8(v, hi, lo);
  packed[frag_id * 128 + lane] = __builtin_bit_cast(u32x4, hi);
  packed[frag_id * 128 + 64 + lane] = __builtin_bit_cast(u32x4, lo);
}
// two fp16 numbers as one dword, `a` in the low half
__device__ __forceinline__ uint32_t pack(_Float16 a, _Float16 b) {
  return (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
}
// four such dwords as a fragment
__device__ __forceinline__ f16x8 frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const u32x4 v = {a, b, c, d};
  return __builtin_bit_cast(f16x8, v);
}
// the product from its parts: acc = sum hi hi, cross = sum (hi lo + lo hi); float or f32x4
template <class T>
__device__ __forceinline__ T combine(T acc, T cross) { return acc + cross * (1.0f / kLoScale); }

}  // namespace ddsp
