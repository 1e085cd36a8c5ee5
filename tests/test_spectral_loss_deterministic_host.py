"""CPU tests of the host side of the reproducible SpectralLoss gradient (SpectralLoss(deterministic=True), the ..._det_f32 entry
points): the slab workspace's size against the formula of include/ddsp_amd.h restated in numpy, the return codes for a missing,
short or misaligned workspace - all of them given before anything is launched, so no GPU is needed - and the keyword's checks."""
import ctypes

import numpy as np
import pytest

from ddsp_amd import _lib, losses
from ddsp_amd import build as build_mod
from test_host_api import test_library_exports_every_symbol_declared_in_the_header  # noqa: F401  (re-run with the new entry points)

DEFAULT_SIZES = (2048, 1024, 512, 256, 128, 64)
POINTS = 4096                          # complex points of a block (kSlPoints)


@pytest.fixture(scope='module')
def lib():
  build_mod.build()
  return _lib.load()


def _c_sizes(sizes):
  return (ctypes.c_int * len(sizes))(*sizes)


def _transform(frame):
  """Points tf.signal.stft transforms for a frame of `frame` samples: the enclosing power of two."""
  return 1 << (int(frame) - 1).bit_length()


def _fused_slab_floats(batch, n, sizes):
  """4 B sum_z nbx_z stretch_z without the 4: a block takes G = max(1, 4096 / S) frames of hop F / 4 and holds (G + 3) hops;
  transforms of 8192 points take one frame per block and hold the frame."""
  total = 0
  for frame in sizes:
    hop = frame // 4
    frames = -(-n // hop)
    s = _transform(frame)
    if s == 8192:
      nbx, stretch = frames, frame
    else:
      g = POINTS // s
      nbx, stretch = -(-frames // g), (g + 3) * hop
    total += batch * nbx * stretch
  return total


@pytest.mark.parametrize('batch,n,sizes', [
    (32, 64000, DEFAULT_SIZES),
    (3, 5001, (4096, 2048, 64, 16)),
    (1, 20000, (8192, 6144, 1024)),
    (2, 3000, (3072, 192, 96)),
])
def test_grad_workspace_bytes_is_the_formula(lib, batch, n, sizes):
  want = 4 * _fused_slab_floats(batch, n, sizes)
  assert lib.ddsp_spectral_loss_grad_workspace_bytes(batch, n, _c_sizes(sizes), len(sizes)) == want
  if (batch, n, sizes) == (32, 64000, DEFAULT_SIZES):
    assert want == 73930752 == 4 * 32 * 63 * 9168


def test_grad_workspace_bytes_is_zero_where_the_loss_workspace_is(lib):
  for batch, n, sizes in ((2, 1000, (100,)), (2, 1000, (64, 8190)), (0, 1000, (64,)), (2, 0, (64,)), (2, 1000, ())):
    assert lib.ddsp_spectral_loss_workspace_bytes(batch, n, _c_sizes(sizes), len(sizes)) == 0
    assert lib.ddsp_spectral_loss_grad_workspace_bytes(batch, n, _c_sizes(sizes), len(sizes)) == 0


def test_one_scale_workspace_bytes(lib):
  """ddsp_stft_mag_backward_workspace_bytes: 2^k frames as above; any other even frame one signal per block - G = 8192 / S frames,
  (G - 1) hop + F floats.  ddsp_stft_frames_mag_backward_workspace_bytes: the same under the caller's geometry."""
  batch, n = 2, 4000
  for frame in (16, 512, 4096):
    assert lib.ddsp_stft_mag_backward_workspace_bytes(batch, n, frame) == 4 * _fused_slab_floats(batch, n, (frame,))
  for frame in (250, 1022, 384, 6144, 8192):
    hop, s = frame // 4, _transform(frame)
    g = 2 * POINTS // s
    frames = -(-n // hop)
    assert lib.ddsp_stft_mag_backward_workspace_bytes(batch, n, frame) == 4 * batch * -(-frames // g) * ((g - 1) * hop + frame)
  for frame in (101, 20, 8194):
    assert lib.ddsp_stft_mag_backward_workspace_bytes(batch, n, frame) == 0
  # the loudness geometry: frames of 2048 every 64, 1024 before the first sample
  n, hop, frames = 8000, 64, 1 + 8000 // 64
  assert lib.ddsp_stft_frames_mag_backward_workspace_bytes(batch, n, 2048, hop, 1024, frames) == 4 * batch * -(-frames // 4) * (3 * hop + 2048)
  assert lib.ddsp_stft_frames_mag_backward_workspace_bytes(batch, n, 2000, hop, 1024, frames) == 0


def test_workspace_return_codes(lib):
  """NULL -> DDSP_ERR_NULL_POINTER (-1); short or misaligned -> DDSP_ERR_WORKSPACE (-4).  The pointers are never followed."""
  batch, n, sizes = 2, 3000, (512, 64)
  c = _c_sizes(sizes)
  p = 1 << 20                                              # stands for a device pointer: 16-byte aligned, never dereferenced
  need = lib.ddsp_spectral_loss_grad_workspace_bytes(batch, n, c, len(sizes))
  part = lib.ddsp_spectral_loss_workspace_bytes(batch, n, c, len(sizes))
  assert need > 0 and part > 0

  def value_and_grad(ws, nbytes):
    return lib.ddsp_spectral_loss_value_and_grad_det_f32(p, p, p, p, p, part, batch, n, c, len(sizes), 1.0, 1.0, ws, nbytes, None)

  def backward(ws, nbytes):
    return lib.ddsp_spectral_loss_backward_det_f32(p, p, p, p, batch, n, c, len(sizes), 1.0, 1.0, ws, nbytes, None)

  one = lib.ddsp_stft_mag_backward_workspace_bytes(batch, n, 512)
  frames = 1 + n // 64
  loud = lib.ddsp_stft_frames_mag_backward_workspace_bytes(batch, n, 2048, 64, 1024, frames)
  assert one > 0 and loud > 0

  def one_scale(ws, nbytes):
    return lib.ddsp_stft_mag_backward_det_f32(p, p, p, ws, nbytes, batch, n, 512, None)

  def loudness(ws, nbytes):
    return lib.ddsp_stft_frames_mag_backward_det_f32(p, p, p, ws, nbytes, batch, n, 2048, 64, 1024, frames, None)

  for call, size in ((value_and_grad, need), (backward, need), (one_scale, one), (loudness, loud)):
    assert call(None, size) == -1, call.__name__
    assert call(p, size - 1) == -4, call.__name__
    assert call(p, 0) == -4, call.__name__
    assert call(p + 4, size + 16) == -4, call.__name__
  # the other arguments are checked as in the atomic entry points
  assert lib.ddsp_spectral_loss_value_and_grad_det_f32(p, p, None, p, p, part, batch, n, c, len(sizes), 1.0, 1.0, p, need, None) == -1
  assert lib.ddsp_spectral_loss_backward_det_f32(p, p, None, p, batch, n, c, len(sizes), 1.0, 1.0, p, need, None) == -1
  assert lib.ddsp_stft_mag_backward_det_f32(p, p, p, p, one, batch, n, 101, None) == -3
  assert lib.ddsp_stft_mag_backward_det_f32(p, p, p, p, one, 0, n, 512, None) == -2


def test_deterministic_keyword():
  for value in ('yes', 1, 0, 'True', 2.0):
    with pytest.raises(ValueError, match='deterministic'):
      losses.SpectralLoss(deterministic=value)
  for value in (None, True, False):
    assert losses.SpectralLoss(deterministic=value).deterministic is value
  assert losses.SpectralLoss().deterministic is None
  # the split into fused and plain scales hands the setting on, also when it changes between calls
  loss = losses.SpectralLoss(fft_sizes=(100, 1000, 64), deterministic=True)
  parts = loss._split_by_kernel([100, 1000])
  assert [part.deterministic for part in parts] == [True, True]
  loss.deterministic = False
  assert [part.deterministic for part in loss._split_by_kernel([100, 1000])] == [False, False]
