// Host side of the reproducible SpectralLoss gradient under the host sanitizers: the workspace arithmetic and the argument checks of
// the ..._det_f32 entry points, which answer before anything is launched - so this runs without a GPU.  A program of its own:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude \
//     tools/spectral_loss_det_host_check.cpp ddsp_amd/csrc/spectral_loss.hip ddsp_amd/csrc/spectral_loss_det.hip \
//     ddsp_amd/csrc/profile.hip -o sl_det_host_check && ./sl_det_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "ddsp_amd.h"

static int failures = 0;
#define EXPECT(what, want) do { const long long got_ = (long long)(what); if (got_ != (long long)(want)) { \
  std::printf("FAIL %s = %lld, expected %lld\n", #what, got_, (long long)(want)); ++failures; } } while (0)

int main() {
  const int sizes[6] = {2048, 1024, 512, 256, 128, 64};
  const int mixed[3] = {8192, 6144, 1024};
  const int bad[1] = {1000};
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(32, 64000, sizes, 6), 73930752ll);
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(128, 64000, sizes, 6), 4 * 73930752ll);
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(65535, 2147483647, sizes, 6) > 0, 1);          // (sizes beyond 2^32 bytes: size_t throughout)
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(1, 20000, mixed, 3), 4ll * (10 * 8192 + 14 * 6144 + 20 * 1792));
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(1, 20000, bad, 1), 0);
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(0, 20000, sizes, 6), 0);
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(1, 0, sizes, 6), 0);
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(1, 100, nullptr, 6), 0);
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(1, 100, sizes, 0), 0);
  EXPECT(ddsp_spectral_loss_grad_workspace_bytes(1, 100, sizes, 17), 0);
  EXPECT(ddsp_stft_mag_backward_workspace_bytes(2, 4000, 250), 4ll * 2 * 3 * (31 * 62 + 250));
  EXPECT(ddsp_stft_mag_backward_workspace_bytes(2, 4000, 101), 0);
  EXPECT(ddsp_stft_mag_backward_workspace_bytes(0, 4000, 256), 0);
  EXPECT(ddsp_stft_frames_mag_backward_workspace_bytes(2, 8000, 2048, 64, 1024, 126), 4ll * 2 * 32 * (3 * 64 + 2048));
  EXPECT(ddsp_stft_frames_mag_backward_workspace_bytes(2, 8000, 2048, 2147483647, 1024, 126), 0);   // a stretch that does not fit an int
  EXPECT(ddsp_stft_frames_mag_backward_workspace_bytes(2, 8000, 2048, 64, 2147483647, 126), 0);
  EXPECT(ddsp_stft_frames_mag_backward_workspace_bytes(2, 8000, 2048, 0, 1024, 126), 0);

  // pointers that are never followed: the calls below all return before a launch
  float* p = reinterpret_cast<float*>(static_cast<uintptr_t>(1) << 20);
  void* ws = p;
  void* crooked = reinterpret_cast<char*>(p) + 4;
  const int B = 2, N = 3000;
  const int two[2] = {512, 64};
  const size_t need = ddsp_spectral_loss_grad_workspace_bytes(B, N, two, 2), part = ddsp_spectral_loss_workspace_bytes(B, N, two, 2);
  EXPECT(ddsp_spectral_loss_value_and_grad_det_f32(p, p, p, p, ws, part, B, N, two, 2, 1.f, 1.f, nullptr, need, nullptr), DDSP_ERR_NULL_POINTER);
  EXPECT(ddsp_spectral_loss_value_and_grad_det_f32(p, p, p, p, ws, part, B, N, two, 2, 1.f, 1.f, ws, need - 1, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_spectral_loss_value_and_grad_det_f32(p, p, p, p, ws, part, B, N, two, 2, 1.f, 1.f, ws, 0, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_spectral_loss_value_and_grad_det_f32(p, p, p, p, ws, part, B, N, two, 2, 1.f, 1.f, crooked, need + 16, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_spectral_loss_value_and_grad_det_f32(p, p, p, p, ws, part, B, N, bad, 1, 1.f, 1.f, ws, need, nullptr), DDSP_ERR_UNSUPPORTED);
  EXPECT(ddsp_spectral_loss_backward_det_f32(p, p, p, p, B, N, two, 2, 1.f, 1.f, nullptr, need, nullptr), DDSP_ERR_NULL_POINTER);
  EXPECT(ddsp_spectral_loss_backward_det_f32(p, p, p, p, B, N, two, 2, 1.f, 1.f, ws, need - 1, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_spectral_loss_backward_det_f32(p, p, p, p, B, N, two, 2, 1.f, 1.f, ws, 0, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_spectral_loss_backward_det_f32(p, p, p, p, B, N, two, 2, 1.f, 1.f, crooked, need + 16, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_spectral_loss_backward_det_f32(p, p, p, p, 0, N, two, 2, 1.f, 1.f, ws, need, nullptr), DDSP_ERR_BAD_SHAPE);
  const size_t one = ddsp_stft_mag_backward_workspace_bytes(B, N, 250);
  EXPECT(ddsp_stft_mag_backward_det_f32(p, p, p, nullptr, one, B, N, 250, nullptr), DDSP_ERR_NULL_POINTER);
  EXPECT(ddsp_stft_mag_backward_det_f32(p, p, p, ws, one - 1, B, N, 250, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_stft_mag_backward_det_f32(p, p, p, ws, 0, B, N, 250, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_stft_mag_backward_det_f32(p, p, p, crooked, one + 16, B, N, 250, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_stft_mag_backward_det_f32(p, p, p, ws, one, B, N, 101, nullptr), DDSP_ERR_UNSUPPORTED);
  const size_t loud = ddsp_stft_frames_mag_backward_workspace_bytes(B, N, 2048, 64, 1024, 47);
  EXPECT(ddsp_stft_frames_mag_backward_det_f32(p, p, p, nullptr, loud, B, N, 2048, 64, 1024, 47, nullptr), DDSP_ERR_NULL_POINTER);
  EXPECT(ddsp_stft_frames_mag_backward_det_f32(p, p, p, ws, loud - 1, B, N, 2048, 64, 1024, 47, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_stft_frames_mag_backward_det_f32(p, p, p, ws, 0, B, N, 2048, 64, 1024, 47, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_stft_frames_mag_backward_det_f32(p, p, p, crooked, loud + 16, B, N, 2048, 64, 1024, 47, nullptr), DDSP_ERR_WORKSPACE);
  EXPECT(ddsp_stft_frames_mag_backward_det_f32(p, p, p, ws, loud, B, N, 2048, 2147483647, 1024, 47, nullptr), DDSP_ERR_UNSUPPORTED);
  std::printf(failures ? "%d checks failed\n" : "host checks ok\n", failures);
  return failures ? 1 : 0;
}
