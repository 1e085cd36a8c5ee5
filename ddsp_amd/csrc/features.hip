// spectral_ops.compute_rms_energy / compute_power (ddsp/spectral_ops.py:223-249) and the decibel conversions of ddsp/core.py:247-277
// for gfx950.  (The mel / log-mel / MFCC kernel sits beside the STFT it extends: csrc/spectral_loss.hip, stft_tq_mel_kernel.)
//
//   frame_energy_kernel   a wavefront per frame: frames of frame_size samples every hop, the first pad_left samples before
//                         sample 0 (spectral_ops.pad 'center': frame_size / 2), zeros outside the row.  No window and no
//                         transform, so any frame size runs.  The reference pads the clip, frames it ([B, frames, frame_size])
//                         and reduces; here a lane walks its share of the frame in sample order and the 64 partial sums meet
//                         in a fixed butterfly: the same bits for a row alone and in a batch.
//   db_convert_kernel     power_to_db / amplitude_to_db / db_to_power / db_to_amplitude, elementwise.
//
// power_to_db is max(10 log10(max(pmin, p)) - ref_db, -range_db) with pmin = 10^(-range_db / 10) (core.py:253-267), the
// arithmetic of loudness_from_mag_kernel; compute_power is amplitude_to_db of the rms energy, and the energy kernel's dB mode
// squares the rms it would have stored, so both routes give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "../../include/ddsp_amd.h"
#include "launch.h"

namespace ddsp {
namespace features {

constexpr int kThreads = 256;
constexpr int kFramesPerBlock = kThreads / kWave;
constexpr float kLn10 = 2.302585092994046f;

__device__ __forceinline__ float power_to_db(float power, float pmin, float ref_db, float range_db) {
  const float db = 10.0f * (logf(max_keep_nan(power, pmin)) / kLn10) - ref_db;       // core.log10: log(x) / log(10)
  return max_keep_nan(db, -range_db);
}

struct EnergyArgs { long rows; int N, n_frames, frame_size, hop, pad_left, db; float inv_size, pmin, ref_db, range_db; };

__global__ __launch_bounds__(kThreads) void frame_energy_kernel(const float* __restrict__ audio, float* __restrict__ out,
                                                                EnergyArgs p) {
  const int lane = threadIdx.x & (kWave - 1);
  const long row = (long)blockIdx.x * kFramesPerBlock + (threadIdx.x >> 6);
  if (row >= p.rows) return;                                    // (wave-uniform)
  const long b = row / p.n_frames;
  const int f = (int)(row - b * p.n_frames);
  const float* __restrict__ x = audio + b * (long)p.N;
  const long first = (long)f * p.hop - p.pad_left;
  float acc = 0.0f;
  for (int i = lane; i < p.frame_size; i += kWave) {
    const long n = first + i;
    const float v = (n >= 0 && n < p.N) ? x[n] : 0.0f;
    acc = fmaf(v, v, acc);
  }
  const float rms = sqrtf(wave_sum(acc) * p.inv_size);
  if (lane == 0) out[row] = p.db ? power_to_db(rms * rms, p.pmin, p.ref_db, p.range_db) : rms;
}

__global__ __launch_bounds__(kThreads) void db_convert_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n, int op,
                                                              float p0, float p1, float pmin) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
    const float x = in[i];
    float y;
    switch (op) {
      case DDSP_DB_POWER_TO_DB: y = power_to_db(x, pmin, p0, p1); break;
      case DDSP_DB_AMPLITUDE_TO_DB: y = power_to_db(x * x, pmin, p0, p1); break;
      case DDSP_DB_TO_POWER: y = expf(x * (kLn10 / 10.0f)); break;            // 10^(db / 10)
      default: y = expf(x * (kLn10 / 20.0f)); break;                          // DDSP_DB_TO_AMPLITUDE: db_to_power(db / 2)
    }
    out[i] = y;
  }
}

static inline float db_floor_power(float range_db) { return (float)pow(10.0, -(double)range_db / 10.0); }

}  // namespace features
}  // namespace ddsp

using namespace ddsp;
using namespace ddsp::features;

extern "C" int ddsp_frame_energy_f32(const float* audio, float* out, int B, int N, int frame_size, int hop, int pad_left, int n_frames,
                                     float ref_db, float range_db, unsigned flags, void* stream) {
  if (!audio || !out) return DDSP_ERR_NULL_POINTER;
  if (B <= 0 || N <= 0 || n_frames <= 0 || hop <= 0 || pad_left < 0 || frame_size <= 0) return DDSP_ERR_BAD_SHAPE;
  if (flags & ~DDSP_ENERGY_DB) return DDSP_ERR_UNSUPPORTED;
  EnergyArgs p;
  p.rows = (long)B * n_frames; p.N = N; p.n_frames = n_frames; p.frame_size = frame_size; p.hop = hop; p.pad_left = pad_left;
  p.db = (flags & DDSP_ENERGY_DB) ? 1 : 0;
  p.inv_size = 1.0f / (float)frame_size; p.pmin = db_floor_power(range_db); p.ref_db = ref_db; p.range_db = range_db;
  const long blocks = (p.rows + kFramesPerBlock - 1) / kFramesPerBlock;
  if (blocks > 0x7fffffffL) return DDSP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(frame_energy_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, audio, out, p);
  return check_launch();
}

extern "C" int ddsp_db_convert_f32(const float* in, float* out, size_t n, int op, float p0, float p1, void* stream) {
  if (!in || !out) return DDSP_ERR_NULL_POINTER;
  if (op < DDSP_DB_POWER_TO_DB || op > DDSP_DB_TO_AMPLITUDE) return DDSP_ERR_UNSUPPORTED;
  if (n == 0) return DDSP_OK;
  const size_t blocks = (n + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(db_convert_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(kThreads), 0, (hipStream_t)stream, in,
                     out, n, op, p0, p1, op <= DDSP_DB_AMPLITUDE_TO_DB ? db_floor_power(p1) : 0.0f);
  return check_launch();
}
