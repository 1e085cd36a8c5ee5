"""The arithmetic of the reference's VectorQuantization (ddsp/training/nn.py:1342-1461) restated with torch ops on the CPU, in fp64
at the fp32 inputs: the split of every row into heads and their concatenation along the batch axis (x_flat, head-major), the
distance matrix |x|^2 - 2 x e^T + |e|^2, its argmin, the embedding lookup, the one-hot counts and sums, the moving averages
without restarts (restart_threshold < 0: nothing is drawn), unquantize and the commitment loss.

THE REFERENCE ITSELF CANNOT RUN HERE: its nn.py imports tensorflow_probability and gin at module level, which are not
installed, and the numpy stand-in behind tests/golden/ carries neither.

Every truth takes dtype= (torch.float64 by default; torch.float32 is the "fp32 mode", the faithful chain in the reference's own
precision, whose error against fp64 sets the tolerance of the GPU tests)."""
import numpy as np
import torch


def _t(x, dtype):
  return x.to(dtype) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype)


def x_flat(x, num_heads, dtype=torch.float64):
  """[..., depth] -> [num_heads * rows, depth / num_heads]: tf.concat(tf.split(x_flat, num_heads, axis=1), axis=0)."""
  x = _t(x, dtype)
  flat = x.reshape(-1, x.shape[-1])
  return torch.cat(torch.split(flat, x.shape[-1] // num_heads, dim=1), 0)


def distances(flat, e):
  return (flat ** 2).sum(1)[:, None] - 2 * torch.matmul(flat, e.T) + (e ** 2).sum(1)[None, :]


def divide_no_nan(sums, counts):
  counts = counts[:, None]
  return torch.where(counts == 0, torch.zeros_like(sums), sums / counts)


def _unflatten(values, shape, num_heads, last):
  """[num_heads * rows, last] (head-major) -> shape[:-1] + (num_heads * last,)"""
  return torch.cat(torch.split(values, values.shape[0] // num_heads, dim=0), 1).reshape(tuple(shape[:-1]) + (num_heads * last,))


def assign(x, e, num_heads=1, dtype=torch.float64):
  """-> (z_q of x's shape, c int64 [..., num_heads], the distance matrix [n, k] in x_flat order)."""
  flat, e = x_flat(x, num_heads, dtype), _t(e, dtype)
  d = distances(flat, e)
  c = torch.argmin(d, dim=1)
  shape = tuple(np.shape(x))
  return _unflatten(e[c], shape, num_heads, e.shape[1]), _unflatten(c[:, None], shape, num_heads, 1), d


def statistics(x, c, k, num_heads=1, dtype=torch.float64):
  """c [..., num_heads] -> (counts [k], sums [k, D]) through the one-hot matrix, as the reference."""
  flat = x_flat(x, num_heads, dtype)
  c = torch.as_tensor(np.asarray(c)).reshape(-1, num_heads).T.reshape(-1)          # x_flat order
  oh = torch.nn.functional.one_hot(c.to(torch.int64), k).to(dtype)
  return oh.sum(0), torch.matmul(oh.T, flat)


def training_step(x, counts, sums, gamma, num_heads=1, dtype=torch.float64):
  """One training call in which nothing restarts -> (z_q, c, new counts, new sums)."""
  counts, sums = _t(counts, dtype), _t(sums, dtype)
  z, c, _ = assign(x, divide_no_nan(sums, counts), num_heads, dtype)
  batch_counts, batch_sums = statistics(x, c, counts.shape[0], num_heads, dtype)
  return z, c, counts - (1 - gamma) * (counts - batch_counts), sums - (1 - gamma) * (sums - batch_sums)


def commitment_loss(z, z_q, weight=0.2, dtype=torch.float64):
  """weight * mean((z - stop_gradient(z_q)) ** 2) and its gradient in z."""
  z = _t(z, dtype).clone().requires_grad_(True)
  loss = weight * ((z - _t(z_q, dtype)) ** 2).mean()
  grad, = torch.autograd.grad(loss, z)
  return loss.detach(), grad
