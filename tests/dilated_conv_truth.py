"""The arithmetic of the reference's DilatedConvStack and DilatedConvDecoder (ddsp/training/nn.py:1153-1323,
ddsp/training/decoders.py:221-285 and the Keras layers they are made of) restated with torch ops on the CPU, in fp64 at the fp32
inputs, as EXPLICIT SHIFTED SUMS: no convolution routine of the framework is called here.

  conv            Conv2D(ch, (K, 1), dilation_rate=(d, 1), padding='same'), optionally behind a ReLU:
                  y[b, t, co] = bias[co] + sum_k sum_ci act(x[b, t + k d - pad_left, ci]) W[k, ci, co], rows outside [0, T) are 0,
                  pad_left = ((K - 1) d) // 2 (TF 'same' at stride 1: the odd row of padding goes behind).
  downsample      Conv2D(ch, (k, 1), (s, 1), padding='same'): out = ceil(T / s), total = max((out - 1) s + k - T, 0),
                  left = total // 2, y[o] = bias + sum_m x[o s + m - left] W[m].
  upsample        Conv2DTranspose(ch, (k, 1), (s, 1), padding='same'), kernel [k, out, in]: the transpose of the downsample that maps
                  T s rows to T: y[j] = bias + full[j + (k - s) // 2], j < T s, full[i s + m] += x[i] W[m]^T.
  stack, decoder  the reference's forward, line for line, over tests/encoder_truth.py's normalisations and tests/decoder_truth.py's
                  Dense.

THE REFERENCE ITSELF CANNOT RUN HERE (no TensorFlow), so the two padding rules are TF's definition
(tensorflow/core/framework/kernel_shape_util.cc GetWindowedOutputSizeVerbose) restated; tests/test_dilated_conv_host.py pins these
sums against F.conv1d / F.conv_transpose1d on the permuted tensor and the upsampler against the adjoint of the downsampler.

Every truth takes dtype= (torch.float64 by default; torch.float32 is the "fp32 mode" whose own error against fp64 sets the
tolerance of the GPU tests); grads is decoder_truth.grads."""
import torch

import decoder_truth as D
import encoder_truth as E

_t = D._t
grads = D.grads


def same_pad_left(taps, dilation):
  return ((taps - 1) * dilation) // 2


def _rows(y, lo, total):
  """y [b, n, c] as rows lo .. lo + n of a [b, total, c] tensor of zeros."""
  b, n, c = y.shape
  return torch.cat([y.new_zeros((b, lo, c)), y, y.new_zeros((b, total - lo - n, c))], dim=1)


def _3d(x, dtype):
  x = _t(x, dtype)
  return (x[:, :, 0, :], True) if x.dim() == 4 else (x, False)


def _kernel(kernel, dtype):
  kernel = _t(kernel, dtype)
  return kernel[:, 0] if kernel.dim() == 4 else kernel


def conv(x, kernel, bias=None, dilation=1, relu_input=False, dtype=torch.float64):
  """x [b, T, ci] or [b, T, 1, ci]; kernel [K, ci, co] or [K, 1, ci, co]; bias [co] or None."""
  x, is_4d = _3d(x, dtype)
  kernel = _kernel(kernel, dtype)
  if relu_input:
    x = torch.relu(x)                                            # gradient 0 at x = 0 and a NaN kept, as tf.nn.relu's
  steps, taps = x.shape[1], kernel.shape[0]
  pad_left = same_pad_left(taps, dilation)
  y = x.new_zeros((x.shape[0], steps, kernel.shape[2]))
  for k in range(taps):
    shift = k * dilation - pad_left                              # y[t] takes x[t + shift]
    lo, hi = max(0, -shift), min(steps, steps - shift)
    if hi > lo:
      y = y + _rows(torch.matmul(x[:, lo + shift:hi + shift], kernel[k]), lo, steps)
  if bias is not None:
    y = y + _t(bias, dtype)
  return y[:, :, None, :] if is_4d else y


def downsample(x, kernel, bias, stride, dtype=torch.float64):
  """kernel [k, ci, co] (or 4-D); [b, T, ci] -> [b, ceil(T / stride), co]."""
  x, is_4d = _3d(x, dtype)
  kernel = _kernel(kernel, dtype)
  steps, taps = x.shape[1], kernel.shape[0]
  out = -(-steps // stride)
  left = max((out - 1) * stride + taps - steps, 0) // 2
  y = x.new_zeros((x.shape[0], out, kernel.shape[2]))
  for m in range(taps):
    rows = [o for o in range(out) if 0 <= o * stride + m - left < steps]
    if rows:
      picked = x[:, [o * stride + m - left for o in rows]]
      y = y + _rows(torch.matmul(picked, kernel[m]), rows[0], out)          # the valid o are one run
  y = y + _t(bias, dtype)
  return y[:, :, None, :] if is_4d else y


def upsample(x, kernel, bias, stride, dtype=torch.float64):
  """kernel [k, co, ci] (or 4-D), the Keras Conv2DTranspose layout; [b, T, ci] -> [b, T stride, co]."""
  x, is_4d = _3d(x, dtype)
  kernel = _kernel(kernel, dtype)
  steps, taps = x.shape[1], kernel.shape[0]
  length = (steps - 1) * stride + taps
  full = x.new_zeros((x.shape[0], length, kernel.shape[1]))
  for m in range(taps):
    part = torch.matmul(x, kernel[m].transpose(0, 1))                        # x[i] lands on row i stride + m
    spread = part.new_zeros((x.shape[0], steps, stride, kernel.shape[1]))
    spread = torch.cat([part[:, :, None, :], spread[:, :, 1:, :]], dim=2).reshape(x.shape[0], steps * stride, -1)
    full = full + _rows(spread[:, :(steps - 1) * stride + 1], m, length)
  before = max(taps - stride, 0) // 2
  y = full[:, before:before + steps * stride] + _t(bias, dtype)
  return y[:, :, None, :] if is_4d else y


def dilations(layers_per_stack, stacks, dilation):
  """The dilation rate of every layer of the stack, as the reference takes it (int() of a power, truncating)."""
  per_stack = [int(dilation ** i) if dilation > 0 else int((-dilation) ** (layers_per_stack - i - 1)) for i in range(layers_per_stack)]
  return per_stack * stacks


def stack(x, z, weights, config, dtype=torch.float64):
  """ddsp/training/nn.py:1287-1323.  weights: dict(conv_in=(kernel, bias), layers=[(kernel, bias) ...], norms=[(scale, shift) or
  (dense kernel, dense bias) ...], resample=[(kernel, bias) ...]); config: dict(dilations, norm_type, conditional, shift_only,
  resample_type, resample_stride, layers_per_resample, resample_after_convolve).  z is None unless conditional."""
  x = E.ensure_4d(_t(x, dtype))
  if config['conditional']:
    z = E.ensure_4d(_t(z, dtype))
  resample = {'downsample': downsample, 'upsample': upsample, None: None}[config['resample_type']]
  per, after = config['layers_per_resample'], config['resample_after_convolve']
  x = conv(x, *weights['conv_in'], dtype=dtype)
  for i, ((kernel, bias), norm) in enumerate(zip(weights['layers'], weights['norms'])):
    if weights['resample'] and not after and i % per == 0:
      x = resample(x, *weights['resample'][i // per], config['resample_stride'], dtype=dtype)
    y = conv(x, kernel, bias, config['dilations'][i], relu_input=True, dtype=dtype)
    if config['conditional']:
      x = x + E.conditional_norm(y, z, norm[0], norm[1], config['norm_type'], config['shift_only'], dtype=dtype)
    else:
      x = x + E.normalize(y, norm[0], norm[1], config['norm_type'], dtype=dtype)
    if weights['resample'] and after and (i + 1) % per == 0:
      x = resample(x, *weights['resample'][i // per], config['resample_stride'], dtype=dtype)
  return x[:, :, 0, :]


def decoder(xs, zs, weights, config, output_splits, dtype=torch.float64):
  """DilatedConvDecoder: xs and zs are the lists of input and conditioning tensors (zs empty when unconditional); weights as
  stack()'s plus dense_out=(kernel, bias).  -> the outputs in output_splits' order."""
  x = torch.cat([_t(v, dtype) for v in xs], dim=-1)
  z = torch.cat([_t(v, dtype) for v in zs], dim=-1) if zs else None
  y = D.dense(stack(x, z, weights, config, dtype=dtype), *weights['dense_out'], dtype=dtype)
  return list(torch.split(y, [n for _, n in output_splits], dim=-1))
