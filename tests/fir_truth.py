"""The truth for the FIR tests: the reference's fft_convolve (ddsp/core.py:1382-1473, crop_and_compensate_delay :1338-1379),
frequency_impulse_response (:1534-1565, apply_window_to_impulse_response :1477-1531), sinc_impulse_response (:1576-1625),
frequency_filter, sinc_filter and exp_sigmoid restated op for op in torch - framed rfft, product, irfft, overlap-add, crop - in
fp64 by default (dtype=torch.float32 is the same chain in the reference's own precision).  Gradients come from torch autograd."""
import math

import numpy as np
import torch


def t(x, dtype=torch.float64):
  return x.to(dtype) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype)


def get_fft_size(frame_size, ir_size):
  return int(2 ** np.ceil(np.log2(ir_size + frame_size - 1)))


def crop_and_compensate_delay(audio, audio_size, ir_size, padding, delay_compensation):
  if padding == 'valid':
    crop_size = ir_size + audio_size - 1
  elif padding == 'same':
    crop_size = audio_size
  else:
    raise ValueError('Padding must be \'valid\' or \'same\', instead of {}.'.format(padding))
  total_size = int(audio.shape[-1])
  crop = total_size - crop_size
  start = (ir_size - 1) // 2 - 1 if delay_compensation < 0 else delay_compensation
  end = crop - start
  return audio[:, start:-end]


def fft_convolve(audio, impulse_response, padding='same', delay_compensation=-1, dtype=torch.float64):
  audio, ir = t(audio, dtype), t(impulse_response, dtype)
  batch_size, audio_size = audio.shape
  if ir.dim() == 2:
    ir = ir[:, None, :]
  if ir.shape[0] == 1 and batch_size > 1:
    ir = ir.expand(batch_size, -1, -1)
  batch_size_ir, n_ir_frames, ir_size = ir.shape
  if batch_size != batch_size_ir:
    raise ValueError('Batch size of audio ({}) and impulse response ({}) must be the same.'.format(batch_size, batch_size_ir))
  frame_size = int(np.ceil(audio_size / n_ir_frames))
  n_audio_frames = -(-audio_size // frame_size)                     # tf.signal.frame(pad_end=True)
  if n_audio_frames != n_ir_frames:
    raise ValueError('Number of Audio frames ({}) and impulse response frames ({}) do not match.'.format(n_audio_frames, n_ir_frames))
  frames = torch.nn.functional.pad(audio, (0, n_audio_frames * frame_size - audio_size)).reshape(batch_size, n_audio_frames, frame_size)
  fft_size = get_fft_size(frame_size, ir_size)
  frames_out = torch.fft.irfft(torch.fft.rfft(frames, fft_size) * torch.fft.rfft(ir, fft_size), fft_size)
  out = torch.zeros((batch_size, (n_audio_frames - 1) * frame_size + fft_size), dtype=dtype)
  for f in range(n_audio_frames):                                   # tf.signal.overlap_and_add
    out = out + torch.nn.functional.pad(frames_out[:, f], (f * frame_size, (n_audio_frames - 1 - f) * frame_size))
  return crop_and_compensate_delay(out, audio_size, ir_size, padding, delay_compensation)


def _raised_cosine(n, a, b, dtype):
  """tf.signal.hann_window / hamming_window (periodic, TensorFlow's default): an odd length divides by n - 1 either way."""
  if n == 1:
    return torch.ones(1, dtype=dtype)
  d = n + (1 - n % 2) - 1
  return a - b * torch.cos(2.0 * math.pi * torch.arange(n, dtype=dtype) / d)


def apply_window_to_impulse_response(ir, window_size=0):
  ir_size = int(ir.shape[-1])
  if window_size <= 0 or window_size > ir_size:
    window_size = ir_size
  window = _raised_cosine(window_size, 0.5, 0.5, ir.dtype)
  padding = ir_size - window_size
  if padding > 0:
    half_idx = (window_size + 1) // 2
    window = torch.cat([window[half_idx:], torch.zeros(padding, dtype=ir.dtype), window[:half_idx]])
  else:
    window = torch.fft.fftshift(window)
  ir = window * ir
  if padding > 0:
    first_half_start = (ir_size - (half_idx - 1)) + 1
    return torch.cat([ir[..., first_half_start:], ir[..., :half_idx + 1]], -1)
  return torch.fft.fftshift(ir, dim=-1)


def frequency_impulse_response(magnitudes, window_size=0, dtype=torch.float64):
  magnitudes = t(magnitudes, dtype)
  ir = torch.fft.irfft(torch.complex(magnitudes, torch.zeros_like(magnitudes)))
  return apply_window_to_impulse_response(ir, window_size)


def exp_sigmoid(x, exponent=10.0, max_value=2.0, threshold=1e-7, dtype=torch.float64):
  return max_value * torch.sigmoid(t(x, dtype)) ** math.log(exponent) + threshold


def frequency_filter(audio, magnitudes, window_size=0, padding='same', dtype=torch.float64):
  return fft_convolve(audio, frequency_impulse_response(magnitudes, window_size, dtype), padding=padding, dtype=dtype)


def sinc(x, threshold=1e-20):
  x = torch.where(x.abs() < threshold, torch.full_like(x, threshold), x)
  x = math.pi * x
  return torch.sin(x) / x


def sinc_normaliser(cutoff_frequency, window_size=512, sample_rate=None, dtype=torch.float64):
  """sum_j w_j s_j, what sinc_impulse_response divides by (about 1 / c): the tests assert that it is far from zero."""
  return _windowed_sinc(t(cutoff_frequency, dtype), window_size, sample_rate)[0].sum(-1)


def _windowed_sinc(cutoff, window_size, sample_rate):
  if cutoff.dim() == 0:
    cutoff = cutoff.reshape(1, 1, 1)
  if sample_rate is not None:
    cutoff = cutoff * (2.0 / float(sample_rate))                     # out of place: the caller's tensor is left alone
  half_size = window_size // 2
  full_size = half_size * 2 + 1
  idx = torch.arange(-half_size, half_size + 1, dtype=cutoff.dtype)[None, None, :]
  return _raised_cosine(full_size, 0.54, 0.46, cutoff.dtype) * sinc(cutoff * idx), half_size


def sinc_impulse_response(cutoff_frequency, window_size=512, sample_rate=None, high_pass=False, dtype=torch.float64):
  ir, half_size = _windowed_sinc(t(cutoff_frequency, dtype), window_size, sample_rate)
  ir = ir / torch.abs(ir.sum(-1, keepdim=True))
  if high_pass:
    pass_through = torch.zeros_like(ir)
    pass_through[..., half_size] = 1.0
    ir = pass_through - ir
  return ir


def sinc_filter(audio, cutoff_frequency, window_size=512, sample_rate=None, padding='same', high_pass=False, dtype=torch.float64):
  ir = sinc_impulse_response(cutoff_frequency, window_size, sample_rate, high_pass, dtype)
  return fft_convolve(audio, ir, padding=padding, dtype=dtype)


def grads(fn, inputs, cotangent, dtype=torch.float64):
  """-> (fn(*inputs) as numpy, [d <fn, cotangent> / d input]) with the inputs taken at their fp32 values."""
  xs = [t(x, dtype).clone().requires_grad_(True) for x in inputs]
  out = fn(*xs)
  got = torch.autograd.grad(out, xs, t(cotangent, dtype).reshape(out.shape), allow_unused=True)
  return out.detach().numpy(), [None if g is None else g.numpy() for g in got]


def finite_difference(fn, inputs, cotangent, which, index, eps):
  """Central difference of <fn, cotangent> along element `index` of inputs[which], fp64."""
  c = t(cotangent)
  def value(delta):
    xs = [t(x).clone() for x in inputs]
    xs[which].reshape(-1)[index] += delta
    return float((fn(*xs) * c).sum())
  return (value(eps) - value(-eps)) / (2.0 * eps)
