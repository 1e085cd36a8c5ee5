"""Truth for losses.wasserstein_distance and WassersteinConsistencyLoss (TEST INFRASTRUCTURE): ddsp/losses.py:584-686 restated
op for op on CPU tensors - two stable argsorts, the sort of the concatenation, searchsorted(right=True), gathers, cumsums.
dtype=torch.float64 is the truth the kernel is measured against (at the fp32 inputs); dtype=torch.float32 is the 'faithful'
mode that stands for the reference's own fp32 arithmetic.  Gradients come from consistency_truth.grads (reverse mode through
this restatement in fp64: sort, gather and cumsum are differentiable, the indices are constants).

Kept as the reference has them: the weights are NOT normalised (the reference computes safe_divide(u_cdf, total) and drops the
result, losses.py:673, 683) - only weights=None gives a CDF that ends at 1; the class computes the distance only with midi=True
and weight > 0, and is the float 0.0 otherwise."""
import numpy as np
import torch

from consistency_truth import _t, grads, hz_to_midi, make_sinusoids  # noqa: F401  (re-exported for the tests)


def _cdf(values, weights, all_values):
  sorter = torch.argsort(values, dim=-1, stable=True)
  indices = torch.searchsorted(torch.gather(values, -1, sorter).detach().contiguous(), all_values[..., :-1].detach().contiguous(),
                               right=True)
  if weights is None:
    return indices.to(values.dtype) / float(values.shape[-1])
  cum = torch.cat([torch.zeros_like(weights)[..., 0:1], torch.cumsum(torch.gather(weights, -1, sorter), dim=-1)], dim=-1)
  return torch.gather(cum, -1, indices)


def wasserstein_distance(u_values, v_values, u_weights, v_weights, p=1.0, dtype=torch.float64):
  u_values, v_values = _t(u_values, dtype), _t(v_values, dtype)
  u_weights = None if u_weights is None else _t(u_weights, dtype)
  v_weights = None if v_weights is None else _t(v_weights, dtype)
  all_values = torch.sort(torch.cat([u_values, v_values], dim=-1), dim=-1, stable=True).values
  deltas = all_values[..., 1:] - all_values[..., :-1]
  u_cdf = _cdf(u_values, u_weights, all_values)
  v_cdf = _cdf(v_values, v_weights, all_values)
  return (deltas * torch.abs(u_cdf - v_cdf) ** p).sum(-1) ** (1.0 / p)


def wasserstein_loss(amps_a, freqs_a, amps_b, freqs_b, weight=1.0, midi=True, dtype=torch.float64):
  loss = 0.0
  if weight > 0.0:
    if midi:
      freqs_a, freqs_b = hz_to_midi(_t(freqs_a, dtype)), hz_to_midi(_t(freqs_b, dtype))
      loss = (weight * wasserstein_distance(freqs_a, freqs_b, amps_a, amps_b, p=1.0, dtype=dtype)).mean()
  return loss


def closed_form_grads(u_values, v_values, u_weights, v_weights, p, cotangent=None):
  """The backward pass the kernel implements, in numpy fp64, for [rows, n] inputs WITH weights:
  S_i = sum_{i' >= i} delta_i' d|D_i'|^p/dD; dW/du_w = S_r, dW/dv_w = -S_r, dW/dall_r = |D_{r-1}|^p - |D_r|^p (each term absent
  at its end), all times 1 / (2 W) for p = 2; r = the stable rank in the concatenation."""
  u_values, v_values, u_weights, v_weights = (np.asarray(x, np.float64) for x in (u_values, v_values, u_weights, v_weights))
  rows, n_u = u_values.shape
  n = n_u + v_values.shape[1]
  out = [np.zeros_like(x) for x in (u_values, v_values, u_weights, v_weights)]
  for row in range(rows):
    allv = np.concatenate([u_values[row], v_values[row]])
    order = np.argsort(allv, kind='stable')
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    wu = np.concatenate([u_weights[row], np.zeros(n - n_u)])[order]
    wv = np.concatenate([np.zeros(n_u), v_weights[row]])[order]
    D = np.cumsum(wu) - np.cumsum(wv)
    delta = np.diff(allv[order])
    W = np.sum(delta * np.abs(D[:-1]) ** p) ** (1.0 / p)
    c = delta * (np.sign(D[:-1]) if p == 1 else 2.0 * D[:-1])
    S = np.concatenate([np.cumsum(c[::-1])[::-1], [0.0]])
    A = np.abs(D) ** p
    gall = np.concatenate([[0.0], A[:-1]]) - np.concatenate([A[:-1], [0.0]])
    coef = (1.0 if cotangent is None else float(np.asarray(cotangent).reshape(-1)[row])) * (1.0 if p == 1 else 1.0 / (2.0 * W))
    out[0][row], out[1][row] = coef * gall[rank[:n_u]], coef * gall[rank[n_u:]]
    out[2][row], out[3][row] = coef * S[rank[:n_u]], -coef * S[rank[n_u:]]
  return out
