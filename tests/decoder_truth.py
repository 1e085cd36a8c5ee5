"""The arithmetic of the reference's RnnFcDecoder (ddsp/training/nn.py:844-934, ddsp/training/decoders.py:27-109 and the Keras
layers they are made of) restated with torch ops on the CPU, in fp64 at the fp32 inputs: Dense, Keras LayerNormalization
(epsilon 1e-3 inside the root, biased variance over the last axis), the activations, the Keras GRU loop (reset_after=True,
gates z, r, h, bias [2, 3 H]), FcStack, and RnnFcDecoder composed of them.

THE REFERENCE ITSELF CANNOT RUN HERE: it needs TensorFlow and Keras, which are not installed, and the numpy stand-in behind
tests/golden/ carries no Keras layers.  tests/test_decoder_host.py pins this restatement against an independent one
(torch.nn.GRU with reordered gates, F.layer_norm, F.leaky_relu) instead.

Every truth takes dtype= (torch.float64 by default; torch.float32 is the "fp32 mode" whose own error against fp64 sets the
tolerance of the GPU tests), and grads() differentiates any of them with autograd, as tests/notes_truth.py does."""
import numpy as np
import torch

EPSILON = 1e-3
ACTIVATIONS = {
    'leaky_relu': lambda x: torch.where(x > 0, x, 0.2 * x),
    'relu': torch.relu,                    # (gradient 0 at 0 as tf.nn.relu's; a NaN stays a NaN, which torch.where(x > 0, x, 0) loses)
    'sigmoid': torch.sigmoid,              # (tf.sigmoid: gradient y (1 - y), 0 at -Inf where 1 / (1 + exp(-x)) differentiates to 0 * Inf)
    'tanh': torch.tanh,
    'linear': lambda x: x,
}


def _t(x, dtype):
  return x.to(dtype) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype)


def dense(x, kernel, bias, dtype=torch.float64):
  return torch.matmul(_t(x, dtype), _t(kernel, dtype)) + _t(bias, dtype)


def layer_norm(x, gamma, beta, dtype=torch.float64):
  x = _t(x, dtype)
  mean = x.mean(-1, keepdim=True)
  var = ((x - mean) ** 2).mean(-1, keepdim=True)
  return (x - mean) / torch.sqrt(var + EPSILON) * _t(gamma, dtype) + _t(beta, dtype)


def bias_norm_act(x, bias, gamma, beta, nonlinearity, dtype=torch.float64):
  """What the kernel fuses: act(LayerNorm(x + bias))."""
  return ACTIVATIONS[nonlinearity](layer_norm(_t(x, dtype) + _t(bias, dtype), gamma, beta, dtype))


def fc(x, w, nonlinearity='leaky_relu', dtype=torch.float64):
  """w = (kernel, bias, gamma, beta)."""
  return ACTIVATIONS[nonlinearity](layer_norm(dense(x, w[0], w[1], dtype), w[2], w[3], dtype))


def fc_stack(x, ws, nonlinearity='leaky_relu', dtype=torch.float64):
  for w in ws:
    x = fc(x, w, nonlinearity, dtype)
  return x


def gru_recurrence(mx, recurrent_kernel, recurrent_bias, h0=None, dtype=torch.float64):
  """The Keras loop on a given mx = x kernel + bias[0]: [batch, time, 3 H] -> all states [batch, time, H]."""
  mx, rk, rb = _t(mx, dtype), _t(recurrent_kernel, dtype), _t(recurrent_bias, dtype)
  hidden = rk.shape[0]
  h = torch.zeros((mx.shape[0], hidden), dtype=dtype) if h0 is None else _t(h0, dtype)
  out = []
  for t in range(mx.shape[1]):
    mh = torch.matmul(h, rk) + rb
    z = torch.sigmoid(mx[:, t, :hidden] + mh[:, :hidden])
    r = torch.sigmoid(mx[:, t, hidden:2 * hidden] + mh[:, hidden:2 * hidden])
    hh = torch.tanh(mx[:, t, 2 * hidden:] + r * mh[:, 2 * hidden:])
    h = z * h + (1.0 - z) * hh
    out.append(h)
  return torch.stack(out, 1)


def gru(x, kernel, recurrent_kernel, bias, h0=None, dtype=torch.float64):
  """tf.keras.layers.GRU(return_sequences=True): kernel [in, 3 H], recurrent_kernel [H, 3 H], bias [2, 3 H]."""
  bias = _t(bias, dtype)
  mx = torch.matmul(_t(x, dtype), _t(kernel, dtype)) + bias[0]
  return gru_recurrence(mx, recurrent_kernel, bias[1], h0, dtype)


def rnn_fc_decoder(inputs, weights, output_splits, state=None, dtype=torch.float64):
  """inputs: the tensors of the input keys (without the state); weights: dict(input_stacks=[[fc weights] ...], gru=(kernel,
  recurrent_kernel, bias), out_stack=[fc weights ...], dense_out=(kernel, bias)).  -> the outputs in output_splits' order,
  then the new state when `state` is given (the stateless form)."""
  stacks = [fc_stack(x, ws, dtype=dtype) for x, ws in zip(inputs, weights['input_stacks'])]
  y = gru(torch.cat(stacks, -1), *weights['gru'], h0=state, dtype=dtype)
  x = fc_stack(torch.cat(stacks + [y], -1), weights['out_stack'], dtype=dtype)
  x = dense(x, *weights['dense_out'], dtype=dtype)
  outs = list(torch.split(x, [n for _, n in output_splits], dim=-1))
  if state is not None:
    outs.append(y[:, -1])
  return outs


def grads(fn, inputs, cotangents):
  """d sum_i <fn(*inputs)[i], cotangents[i]> / d inputs, in fp64: a list of numpy arrays, one per input."""
  leaves = [torch.as_tensor(np.asarray(v), dtype=torch.float64).clone().requires_grad_(True) for v in inputs]
  outs = fn(*leaves)
  outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
  total = sum((o * torch.as_tensor(np.asarray(c), dtype=torch.float64)).sum() for o, c in zip(outs, cotangents))
  return [g.numpy() for g in torch.autograd.grad(total, leaves)]
