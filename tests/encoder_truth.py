"""The arithmetic of the reference's normalisations and z encoders (ddsp/training/nn.py:561-603 and 1075-1136,
ddsp/training/encoders.py:27-126 and 286-334) restated with torch ops on the CPU, in fp64 at the fp32 inputs: normalize_op
(reshape to groups, tf.nn.moments over height, width and the group's channels, subtract, divide by sqrt(var + eps)), Normalize,
ConditionalNorm, and the encoder chains DOWNSTREAM of the MFCCs (instance norm -> GRU -> Dense -> resample).  The GRU and Dense
are tests/decoder_truth.py's; the resampler is the oracle's (oracle/ddsp_oracle.py resample), applied to the identity: resampling
is linear, so its matrix restates it exactly and autograd can go through it.

THE REFERENCE ITSELF CANNOT RUN HERE (no TensorFlow); tests/test_encoder_host.py pins normalize_op against
torch.nn.functional.group_norm on the permuted tensor instead.

Every truth takes dtype= (torch.float64 by default; torch.float32 is the "fp32 mode" whose own error against fp64 sets the
tolerance of the GPU tests); decoder_truth.grads differentiates any of them."""
import functools

import numpy as np
import torch

import decoder_truth as D
from oracle import ddsp_oracle as O

EPS = 1e-5
N_GROUPS = {'instance': lambda ch: ch, 'layer': lambda ch: 1, 'group': lambda ch: 32}
_t = D._t
grads = D.grads


def normalize_op(x, norm_type='layer', eps=EPS, dtype=torch.float64):
  x = _t(x, dtype)
  if norm_type is None:
    return x
  shape = x.shape
  n_groups = N_GROUPS[norm_type](shape[-1])
  x = x.reshape(tuple(shape[:-1]) + (n_groups, shape[-1] // n_groups))
  mean = x.mean(dim=(1, 2, 4), keepdim=True)
  var = ((x - mean) ** 2).mean(dim=(1, 2, 4), keepdim=True)
  x = (x - mean) / torch.sqrt(var + eps)
  return x.reshape(shape)


def ensure_4d(x):
  if x.dim() == 2:
    return x[:, None, None, :]
  if x.dim() == 3:
    return x[:, :, None, :]
  return x


def inv_ensure_4d(x, n_dims):
  if n_dims == 2:
    return x[:, 0, 0, :]
  if n_dims == 3:
    return x[:, :, 0, :]
  return x


def normalize(x, scale, shift, norm_type='layer', dtype=torch.float64):
  """The Normalize layer: scale, shift [1, 1, 1, ch]."""
  x = _t(x, dtype)
  n_dims = x.dim()
  x = normalize_op(ensure_4d(x), norm_type, dtype=dtype)
  return inv_ensure_4d(x * _t(scale, dtype) + _t(shift, dtype), n_dims)


def conditional_norm(x, z, kernel, bias, norm_type='instance', shift_only=False, dtype=torch.float64):
  x = normalize_op(x, norm_type, dtype=dtype)
  ch = x.shape[-1]
  scale_shift = D.dense(z, kernel, bias, dtype)
  if shift_only:
    return x + scale_shift
  return x * scale_shift[..., :ch] + scale_shift[..., ch:]


@functools.lru_cache(maxsize=None)
def resample_matrix(n_frames, n_timesteps, method='linear', add_endpoint=True):
  """[n_timesteps, n_frames] in fp64: the oracle's resample of the identity."""
  eye = np.eye(n_frames, dtype=np.float64)[:, :, None]                     # [batch = frame, time, 1]
  return np.ascontiguousarray(O.resample(eye, n_timesteps, method=method, add_endpoint=add_endpoint, dtype=np.float64)[:, :, 0].T)


def resample(x, n_timesteps, method='linear', add_endpoint=True, dtype=torch.float64):
  """[batch, n_frames, ch] -> [batch, n_timesteps, ch]."""
  x = _t(x, dtype)
  matrix = torch.as_tensor(resample_matrix(int(x.shape[1]), int(n_timesteps), method, add_endpoint)).to(dtype)
  return torch.einsum('nf,bfc->bnc', matrix, x)


def expand_z(z, time_steps, dtype=torch.float64):
  if z.dim() == 2:
    z = z[:, None, :]
  return z if int(z.shape[1]) == time_steps else resample(z, time_steps, dtype=dtype)


def mfcc_rnn_encoder(mfccs, scale, shift, kernel, recurrent_kernel, bias, dense_kernel, dense_bias, time_steps, dtype=torch.float64):
  """MfccTimeDistributedRnnEncoder downstream of compute_mfcc: mfccs [batch, frames, 30] -> z [batch, time_steps, z_dims]."""
  z = normalize(_t(mfccs, dtype)[:, :, None, :], scale, shift, 'instance', dtype)[:, :, 0, :]
  z = D.gru(z, kernel, recurrent_kernel, bias, dtype=dtype)
  z = D.dense(z, dense_kernel, dense_bias, dtype)
  return expand_z(z, time_steps, dtype)


def mfcc_encoder(mfccs, scale, shift, time_steps, dtype=torch.float64):
  """MfccEncoder downstream of its (already resampled, concatenated) MFCCs."""
  z = normalize(_t(mfccs, dtype)[:, :, None, :], scale, shift, 'instance', dtype)[:, :, 0, :]
  return expand_z(z, time_steps, dtype)


def aggregate_features_encoder(f0_scaled, ld_scaled, kernel, bias, time_steps, dtype=torch.float64):
  x = torch.cat([_t(f0_scaled, dtype), _t(ld_scaled, dtype)], -1)
  z = D.dense(x, kernel, bias, dtype).mean(dim=1, keepdim=True)
  return expand_z(z, time_steps, dtype)
