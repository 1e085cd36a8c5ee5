"""Truth for losses.HmmTranscriber (TEST INFRASTRUCTURE): the DENSE hidden Markov model, built exactly as the constructor at
ddsp/losses.py:275-304 builds it (uniform initial distribution; (hold - other) * eye + other * ones, rows renormalised; a
MultivariateNormalDiag over (pitch, amps) per state), with the forward algorithm and Viterbi written from their definitions
on CPU tensors: a logsumexp, or a max with its argmax, over a [batch, states, states] tensor per step.

NO GOLDEN VECTORS COME FROM THE REFERENCE: its class derives from tfp.distributions.HiddenMarkovModel, TensorFlow Probability
cannot be imported where the fixtures are made, and the numpy stand-in for TensorFlow the other fixtures were made with has no
TFP.  So this restatement is the truth, and tests/test_hmm_host.py validates it by enumerating every path of small models.

dtype=torch.float64 is the truth the kernels are measured against (at the fp32 inputs), and gradients come from reverse mode
through it (consistency_truth.grads); dtype=torch.float32 is the 'faithful' mode: the same dense recursion op by op in fp32,
which stands for the reference's own arithmetic."""
import math

import numpy as np
import torch

from consistency_truth import _t, grads  # noqa: F401  (re-exported for the tests)

DEFAULTS = dict(avg_length=200, midi_std=0.5, amps_on_center=1.5, amps_on_scale=0.5, amps_off_center=0.0, amps_off_scale=0.1)


class Model:
  """The three distributions of the constructor as dense tensors of `dtype`."""

  def __init__(self, n_pitches=128, dtype=torch.float64, **kwargs):
    k = dict(DEFAULTS, **kwargs)
    n = n_pitches
    self.n_pitches, self.dtype = n, dtype
    self.log_initial = torch.log(torch.ones(n, dtype=dtype) / n)
    hold = 1.0 - 1.0 / k['avg_length']
    other = (1.0 - hold) / (n - 1)
    transitions = (hold - other) * torch.eye(n, dtype=dtype) + other * torch.ones(n, n, dtype=dtype)
    transitions = transitions / transitions.sum(dim=1, keepdim=True)
    self.log_transitions = torch.log(transitions)                                      # [from, to]
    one = torch.ones(1, dtype=dtype)
    self.pitch_loc = torch.cat([one * n / 2.0, torch.arange(1, n, dtype=dtype)])
    self.pitch_scale = torch.cat([one * n, torch.ones(n - 1, dtype=dtype) * k['midi_std']])
    self.amps_loc = torch.cat([one * k['amps_off_center'], torch.ones(n - 1, dtype=dtype) * k['amps_on_center']])
    self.amps_scale = torch.cat([one * k['amps_off_scale'], torch.ones(n - 1, dtype=dtype) * k['amps_on_scale']])

  def log_obs(self, pitch, amps):
    """MultivariateNormalDiag(loc, scale_diag).log_prob of (pitch, amps) [batch, steps, 1] -> [batch, steps, states]."""
    pitch, amps = _t(pitch, self.dtype), _t(amps, self.dtype)
    zp, za = (pitch - self.pitch_loc) / self.pitch_scale, (amps - self.amps_loc) / self.amps_scale
    return -0.5 * (zp * zp + za * za) - torch.log(self.pitch_scale) - torch.log(self.amps_scale) - math.log(2.0 * math.pi)


def log_prob(pitch, amps, n_pitches=128, dtype=torch.float64, **kwargs):
  """HiddenMarkovModel.log_prob: the forward algorithm in log space -> [batch]."""
  m = Model(n_pitches, dtype, **kwargs)
  obs = m.log_obs(pitch, amps)
  alpha = m.log_initial + obs[:, 0]
  for t in range(1, obs.shape[1]):
    alpha = torch.logsumexp(alpha[:, :, None] + m.log_transitions, dim=1) + obs[:, t]
  return torch.logsumexp(alpha, dim=-1)


def nll(pitch, amps, n_pitches=128, weight=1.0, per_example_loss=False, dtype=torch.float64, **kwargs):
  """HmmTranscriber.nll (ddsp/losses.py:331-336)."""
  avg_nll = -log_prob(pitch, amps, n_pitches, dtype, **kwargs) / np.shape(pitch)[1]
  return weight * (avg_nll if per_example_loss else avg_nll.mean())


def viterbi(pitch, amps, n_pitches=128, dtype=torch.float64, **kwargs):
  """HiddenMarkovModel.posterior_mode -> (path [batch, steps] int64, its score [batch]); argmax takes the lowest index."""
  m = Model(n_pitches, dtype, **kwargs)
  obs = m.log_obs(pitch, amps)
  v = m.log_initial + obs[:, 0]
  back = []
  for t in range(1, obs.shape[1]):
    v, arg = torch.max(v[:, :, None] + m.log_transitions, dim=1)
    v = v + obs[:, t]
    back.append(arg)
  score, state = torch.max(v, dim=-1)
  path = [state]
  for arg in reversed(back):
    state = torch.gather(arg, 1, state[:, None])[:, 0]
    path.append(state)
  return torch.stack(path[::-1], dim=1), score


def path_score(path, pitch, amps, n_pitches=128, **kwargs):
  """log p(path, observations) in fp64 -> [batch]."""
  m = Model(n_pitches, torch.float64, **kwargs)
  path = torch.as_tensor(np.asarray(path), dtype=torch.int64)
  obs = torch.gather(m.log_obs(pitch, amps), 2, path[:, :, None])[:, :, 0]
  return m.log_initial[path[:, 0]] + obs.sum(-1) + m.log_transitions[path[:, :-1], path[:, 1:]].sum(-1)


def make_notes(rng, batch, steps, n_pitches):
  """Note-like fp32 (pitch, amps) [batch, steps, 1]: segments of 3-40 steps (2-5 where the case has fewer than 40 steps, so
  that the decoded path changes state); a segment is a note with probability 0.75 - an integer pitch in 1 .. n_pitches - 1
  with +-0.3 of jitter, amps 1.5 +- 0.3 - and silence otherwise: amps near 0, pitch uniform over the range."""
  lo, hi = (2, 5) if steps < 40 else (3, 40)
  pitch, amps = np.zeros((batch, steps)), np.zeros((batch, steps))
  for b in range(batch):
    t = 0
    while t < steps:
      length = min(int(rng.integers(lo, hi + 1)), steps - t)
      if rng.uniform() < 0.75:
        pitch[b, t:t + length] = rng.integers(1, n_pitches) + rng.uniform(-0.3, 0.3, length)
        amps[b, t:t + length] = 1.5 + rng.uniform(-0.3, 0.3, length)
      else:
        pitch[b, t:t + length] = rng.uniform(0.0, n_pitches, length)
        amps[b, t:t + length] = rng.normal(0.0, 0.03, length)
      t += length
  return pitch.astype(np.float32)[:, :, None], amps.astype(np.float32)[:, :, None]
