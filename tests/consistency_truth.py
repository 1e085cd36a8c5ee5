"""Truth for the consistency losses and core.sinusoidal_to_harmonic (TEST INFRASTRUCTURE): ddsp/losses.py:489-578, 689-1076 and
ddsp/core.py:733-781 restated in the reference's op order on CPU tensors.  dtype=torch.float64 is the truth the kernels are
measured against (at the fp32 inputs); dtype=torch.float32 is the 'faithful' mode that stands for the reference's own fp32
arithmetic.  Gradients come from reverse-mode differentiation of this restatement in fp64 (exact derivatives of the same
ops, tf.where / safe_divide branches included); tests/test_consistency_host.py checks them against central differences."""
import math

import numpy as np
import torch


def _t(x, dtype):
  return torch.as_tensor(np.asarray(x), dtype=dtype) if not isinstance(x, torch.Tensor) else x.to(dtype)


def safe_divide(num, den, eps=1e-7):
  return num / torch.where(den == 0.0, torch.full_like(den, eps), den)


def hz_to_midi(f):
  safe = torch.where(f <= 0.0, torch.full_like(f, 1e-5), f)
  notes = 12.0 * (torch.log(safe) / math.log(2.0) - math.log(440.0) / math.log(2.0)) + 69.0
  return torch.where(f <= 0.0, torch.zeros_like(f), notes)


def _mixture_log_prob(x, mu, log_w, scale):
  """MixtureSameFamily(Categorical(logits=log_w), Normal(mu, scale)).log_prob(x): x [..., 1] against mu, log_w [..., J]."""
  log_w = log_w - torch.logsumexp(log_w, dim=-1, keepdim=True)
  z = (x - mu) / scale
  lp = -0.5 * z * z - math.log(scale) - 0.5 * math.log(2.0 * math.pi)
  return torch.logsumexp(lp + log_w, dim=-1)


def sinusoidal_to_harmonic(sin_amps, sin_freqs, f0_hz, harmonic_width=0.1, n_harmonics=100, sample_rate=16000, normalize=False,
                           dtype=torch.float64):
  sin_amps, sin_freqs, f0_hz = _t(sin_amps, dtype), _t(sin_freqs, dtype), _t(f0_hz, dtype)
  n = torch.arange(1, n_harmonics + 1, dtype=dtype)
  # the Nyquist decision is taken on the fp32 product, as every mode of the reference takes it
  harm_freqs = f0_hz * n
  masked = (f0_hz.detach().to(torch.float32) * n.to(torch.float32)) >= sample_rate / 2.0
  diff = sin_freqs[:, :, None, :] - harm_freqs[..., None]
  ratio = torch.abs(safe_divide(diff, f0_hz[..., None]))
  weights = torch.exp(-(ratio / harmonic_width) ** 2.0)
  if normalize:
    wsum = weights.sum(-1, keepdim=True)
    # (the branch not taken is given a divisor of 1: the same function, and no inf * 0 in its derivative where a sum is tiny)
    weights = torch.where(wsum > 1.0, weights / torch.where(wsum > 1.0, wsum, torch.ones_like(wsum)), weights)
  harm_amps = (weights * sin_amps[:, :, None, :]).sum(-1)
  harm_amps = torch.where(masked, torch.zeros_like(harm_amps), harm_amps)
  harm_amp = harm_amps.sum(-1, keepdim=True)
  return harm_amp, safe_divide(harm_amps, harm_amp)


def kde_nll(amps, freqs, amps_target, freqs_target, scale, dtype=torch.float64):
  amps, freqs, amps_target, freqs_target = (_t(v, dtype) for v in (amps, freqs, amps_target, freqs_target))
  mu = hz_to_midi(freqs_target)
  at = torch.where(amps_target == 0.0, torch.full_like(amps_target, 1e-7), amps_target)
  an = safe_divide(at, at.sum(-1, keepdim=True))
  x = hz_to_midi(freqs)
  nll = -_mixture_log_prob(x[..., None], mu[:, :, None, :], torch.log(an)[:, :, None, :], scale)
  amps_norm = safe_divide(amps, amps.sum(-1, keepdim=True))
  return (nll * amps_norm).mean(-1)


def kde_loss(amps_a, freqs_a, amps_b, freqs_b, weight_a=1.0, weight_b=1.0, weight_mean_amp=1.0, scale_a=0.1, scale_b=0.1,
             dtype=torch.float64):
  amps_a, freqs_a, amps_b, freqs_b = (_t(v, dtype) for v in (amps_a, freqs_a, amps_b, freqs_b))
  loss = torch.zeros((), dtype=dtype)
  if weight_a > 0.0:
    loss = loss + (weight_a * kde_nll(amps_a, freqs_a, amps_b, freqs_b, scale_b, dtype)).mean()
  if weight_b > 0.0:
    loss = loss + (weight_b * kde_nll(amps_b, freqs_b, amps_a, freqs_a, scale_a, dtype)).mean()
  if weight_mean_amp > 0.0:
    loss = loss + weight_mean_amp * torch.abs(amps_a.mean(-1) - amps_b.mean(-1)).mean()
  return loss


def twm_loss_tensors(f0_candidates, freqs, amps, sinusoids_scale=0.5, harmonics_scale=0.2, n_harmonic_points=10,
                     n_harmonic_gaussians=30, sample_rate=16000, dtype=torch.float64):
  f0c, freqs, amps = _t(f0_candidates, dtype), _t(freqs, dtype), _t(amps, dtype)
  G, P = n_harmonic_gaussians, n_harmonic_points
  loc = torch.arange(1, G + 1, dtype=dtype)
  ratios = safe_divide(freqs[:, :, None, :], f0c[:, :, :, None])                       # [b, t, c, k]
  nll_s = -_mixture_log_prob(ratios[..., None], loc, torch.full((G,), 1.0 / G, dtype=dtype), harmonics_scale)
  a = amps[:, :, None, :]
  sinusoids_loss = safe_divide((nll_s * a).sum(-1), a.sum(-1))
  mu = hz_to_midi(freqs)
  ap = torch.where(amps == 0.0, torch.full_like(amps, 1e-7), amps)
  an = safe_divide(ap, ap.sum(-1, keepdim=True))
  n = torch.arange(1, P + 1, dtype=dtype)
  # fl32(f0 n): the reference rounds the product to fp32 before hz_to_midi; the truth keeps the fp32 inputs' exact product
  # unless that changes the side of Nyquist (the mask below is taken on the fp32 product in every mode)
  harmonics = hz_to_midi(f0c[..., None] * n)                                               # [b, t, c, p]
  nll_h = -_mixture_log_prob(harmonics[..., None], mu[:, :, None, None, :], torch.log(an)[:, :, None, None, :], sinusoids_scale)
  prior = torch.linspace(1.0, 1.0 / P, P, dtype=dtype)
  h_loss = nll_h * prior
  hz32 = f0c.detach().to(torch.float32)[..., None] * n.to(torch.float32)
  mask = (hz32 < sample_rate / 2.0).to(dtype)
  h_loss = h_loss * safe_divide(mask, mask.mean(-1, keepdim=True))
  return sinusoids_loss, h_loss.mean(-1)


def twm_loss(f0_candidates, freqs, amps, sinusoids_weight=1.0, harmonics_weight=1.0, softmin_temperature=1.0, dtype=torch.float64, **kw):
  s, h = twm_loss_tensors(f0_candidates, freqs, amps, dtype=dtype, **kw)
  L = sinusoids_weight * s + harmonics_weight * h
  return (L * torch.softmax(-L / softmin_temperature, dim=-1)).mean()


def mean_difference(target, value, loss_type='L1', weights=None):
  d = target - value
  w = 1.0 if weights is None else weights
  return torch.abs(d * w).mean() if loss_type == 'L1' else (d ** 2 * w).mean()


def amp_loss(amp, amp_target, loss_type='L1', weights=None, log=False, amin=1e-5, dtype=torch.float64):
  amp, amp_target = _t(amp, dtype), _t(amp_target, dtype)
  if log:
    amp = torch.log(torch.clamp(amp, min=amin)) / math.log(10.0)
    amp_target = torch.log(torch.clamp(amp_target, min=amin)) / math.log(10.0)
  return mean_difference(amp, amp_target, loss_type, None if weights is None else _t(weights, dtype))


def freq_loss(f_hz, f_hz_target, loss_type='L1', weights=None, dtype=torch.float64):
  return mean_difference(hz_to_midi(_t(f_hz, dtype)), hz_to_midi(_t(f_hz_target, dtype)), loss_type,
                         None if weights is None else _t(weights, dtype))


def harmonic_consistency(harm_amp, harm_amp_target, harm_dist, harm_dist_target, f0_hz, f0_hz_target, amp_weight=1.0, dist_weight=1.0,
                         f0_weight=1.0, amp_threshold=1e-4, dtype=torch.float64):
  w = (_t(harm_amp_target, torch.float32) >= np.float32(amp_threshold)).to(dtype)
  return {'harm_amp_loss': amp_weight * amp_loss(harm_amp, harm_amp_target, dtype=dtype),
          'harm_dist_loss': dist_weight * amp_loss(harm_dist, harm_dist_target, weights=w, dtype=dtype),
          'f0_hz_loss': f0_weight * freq_loss(f0_hz, f0_hz_target, weights=w, dtype=dtype)}


def grads(fn, inputs, cotangents=None):
  """fp64 gradients of fn(*inputs) (a tensor or a tuple of tensors; contracted with `cotangents`, ones by default)."""
  xs = [torch.as_tensor(np.asarray(v), dtype=torch.float64).clone().requires_grad_(True) for v in inputs]
  out = fn(*xs)
  outs = out if isinstance(out, (tuple, list)) else (out,)
  cots = cotangents if cotangents is not None else [np.ones(tuple(o.shape)) for o in outs]
  total = sum((o * torch.as_tensor(np.asarray(c), dtype=torch.float64)).sum() for o, c in zip(outs, cots))
  return [g.numpy() if g is not None else np.zeros(tuple(x.shape)) for g, x in zip(torch.autograd.grad(total, xs, allow_unused=True), xs)]


def make_sinusoids(rng, b, t, k, sample_rate=16000, zeros=False, wide=False):
  """Random fp32 sinusoids: log-uniform frequencies (`wide`: from 0 Hz to above Nyquist), amplitudes in (0, 1] (`zeros`: some 0)."""
  hi = sample_rate / 2.0
  freqs = np.exp(rng.uniform(np.log(40.0), np.log(hi * (1.3 if wide else 0.95)), (b, t, k)))
  if wide:
    freqs[rng.uniform(size=freqs.shape) < 0.05] = 0.0
  amps = rng.uniform(0.01, 1.0, (b, t, k))
  if zeros:
    amps[rng.uniform(size=amps.shape) < 0.2] = 0.0
    if b * t > 1:
      amps[0, 0] = 0.0                       # a frame of zeros alone (not the only frame of a case)
  return amps.astype(np.float32), freqs.astype(np.float32)
