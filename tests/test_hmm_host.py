"""CPU tests of losses.HmmTranscriber (no kernel runs): the truth helper (tests/hmm_truth.py) against the enumeration of every
path of small models, the structured recursions the kernels implement against the dense truth, the constructor's attributes
and defaults, the errors raised before any launch, and straight_through."""
import inspect
import itertools

import numpy as np
import pytest
import torch

import hmm_truth as T
from ddsp_amd import _lib, core, losses


def _brute_force(pitch, amps, n_pitches, **kwargs):
  """-> (log p(observations), the most likely path) per batch row, from all n_pitches ** steps paths; among equally likely
  paths the first in lexicographic order."""
  m = T.Model(n_pitches, torch.float64, **kwargs)
  obs = m.log_obs(pitch, amps).numpy()
  log_init, log_trans = m.log_initial.numpy(), m.log_transitions.numpy()
  steps = obs.shape[1]
  log_probs, paths = [], []
  for row in obs:
    scores = []
    for path in itertools.product(range(n_pitches), repeat=steps):
      score = log_init[path[0]] + row[0, path[0]]
      for t in range(1, steps):
        score += log_trans[path[t - 1], path[t]] + row[t, path[t]]
      scores.append((score, path))
    top = max(s for s, _ in scores)
    log_probs.append(top + np.log(sum(np.exp(s - top) for s, _ in scores)))
    paths.append(next(p for s, p in scores if s == top))
  return np.array(log_probs), np.array(paths)


@pytest.mark.parametrize('n_pitches,steps', [(3, 5), (2, 6)])
def test_truth_against_all_paths(n_pitches, steps):
  rng = np.random.default_rng(100 * n_pitches + steps)
  pitch, amps = T.make_notes(rng, 3, steps, n_pitches)
  for kwargs in ({}, dict(avg_length=3, midi_std=1.0, amps_off_scale=0.4)):
    want_lp, want_path = _brute_force(pitch, amps, n_pitches, **kwargs)
    np.testing.assert_allclose(T.log_prob(pitch, amps, n_pitches, **kwargs).numpy(), want_lp, rtol=1e-12)
    path, score = T.viterbi(pitch, amps, n_pitches, **kwargs)
    assert np.array_equal(path.numpy(), want_path)
    np.testing.assert_allclose(score.numpy(), T.path_score(want_path, pitch, amps, n_pitches, **kwargs).numpy(), rtol=1e-12)
    np.testing.assert_allclose(T.nll(pitch, amps, n_pitches, weight=0.5, **kwargs).numpy(), -0.5 * want_lp.mean() / steps, rtol=1e-12)


def _structured(pitch, amps, n_pitches, **kwargs):
  """The recursions of csrc/hmm.hip in fp64 numpy: O(states) a step.  -> (log_prob, path)."""
  k = dict(T.DEFAULTS, **kwargs)
  hold = 1.0 - 1.0 / k['avg_length']
  other = (1.0 - hold) / (n_pitches - 1)
  obs = T.Model(n_pitches, torch.float64, **kwargs).log_obs(pitch, amps).numpy()
  log_probs, paths = [], []
  for row in obs:
    alpha, scale = np.exp(row[0] - row[0].max()) / n_pitches, row[0].max()
    v, stayed, args = row[0].copy(), [], []
    for o in row[1:]:
      alpha = (other * alpha.sum() + (hold - other) * alpha) * np.exp(o - o.max())
      scale += o.max() + np.log(alpha.sum())
      alpha = alpha / alpha.sum()
      arg = int(np.argmax(v))
      stay, jump = v + np.log(hold), v[arg] + np.log(other)
      stayed.append((stay > jump) | ((stay == jump) & (np.arange(n_pitches) <= arg)))
      args.append(arg)
      v = np.maximum(stay, jump) + o
    log_probs.append(scale + np.log(alpha.sum()))
    path = [int(np.argmax(v))]
    for keep, arg in zip(reversed(stayed), reversed(args)):
      path.append(path[-1] if keep[path[-1]] else arg)
    paths.append(path[::-1])
  return np.array(log_probs), np.array(paths)


@pytest.mark.parametrize('n_pitches,steps', [(2, 1), (5, 7), (128, 64), (200, 100)])
def test_structured_recursions_are_the_dense_ones(n_pitches, steps):
  """other * 1 + (hold - other) * I: the forward step is a sum and a scale, the Viterbi step a max against the best jump."""
  rng = np.random.default_rng(1000 * n_pitches + steps)
  pitch, amps = T.make_notes(rng, 2, steps, n_pitches)
  got_lp, got_path = _structured(pitch, amps, n_pitches)
  np.testing.assert_allclose(got_lp, T.log_prob(pitch, amps, n_pitches).numpy(), rtol=1e-12)
  assert np.array_equal(got_path, T.viterbi(pitch, amps, n_pitches)[0].numpy())


def test_constructor_matches_the_reference():
  params = [(p.name, p.default) for p in inspect.signature(losses.HmmTranscriber).parameters.values()]
  assert params == [('avg_length', 200), ('midi_std', 0.5), ('amps_on_center', 1.5), ('amps_on_scale', 0.5), ('amps_off_center', 0.0),
                    ('amps_off_scale', 0.1), ('n_timesteps', 1000), ('n_pitches', 128), ('weight', 1.0)]
  hmm = losses.HmmTranscriber()
  assert (hmm.avg_length, hmm.midi_std, hmm.n_timesteps, hmm.n_pitches, hmm.weight) == (200, 0.5, 1000, 128, 1.0)
  hmm = losses.HmmTranscriber(avg_length=20, midi_std=1.0, n_timesteps=64, n_pitches=32, weight=0.25)
  assert (hmm.avg_length, hmm.midi_std, hmm.n_timesteps, hmm.n_pitches, hmm.weight) == (20, 1.0, 64, 32, 0.25)
  n, hold, other = hmm._model[:3]
  assert n == 32 and abs(hold + 31 * other - 1.0) < 1e-15 and abs(hold - 0.95) < 1e-15
  params = lambda fn: [(p.name,) if p.default is inspect.Parameter.empty else (p.name, p.default)
                       for p in inspect.signature(fn).parameters.values() if p.name != 'self']
  assert params(losses.HmmTranscriber.nll) == [('pitch',), ('amps',), ('per_example_loss', False)]
  assert params(losses.HmmTranscriber.predict_midi) == [('pitch',), ('amps',), ('channel_dim', True), ('dtype', torch.float32)]
  assert 'out of scope' in losses.HmmTranscriber.__doc__.lower()


@pytest.fixture
def on_cpu(monkeypatch):
  """The shape checks run before any kernel: let tensors stay on the CPU, and let no library load."""
  def no_library():
    raise AssertionError('the library must not be loaded here')
  monkeypatch.setattr(_lib, 'load', no_library)
  monkeypatch.setattr(core, '_device', lambda: torch.device('cpu'))
  monkeypatch.setattr(core, 'tf_float32', lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32).contiguous()
                      if not isinstance(x, torch.Tensor) else x.to(torch.float32).contiguous())


def test_value_errors_are_raised_before_any_launch(on_cpu):
  hmm = losses.HmmTranscriber(n_timesteps=8, n_pitches=16)
  z = torch.zeros
  for call in (hmm, hmm.nll, hmm.predict_midi):
    with pytest.raises(ValueError, match='n_timesteps = 8.*got 9'):
      call(z(2, 9, 1), z(2, 9, 1))
    with pytest.raises(ValueError, match=r'\(2, 8, 1\).*\(3, 8, 1\)'):
      call(z(2, 8, 1), z(3, 8, 1))
    with pytest.raises(ValueError, match=r'\(2, 8, 1\).*\(2, 7, 1\)'):
      call(np.zeros((2, 8, 1)), z(2, 7, 1))


def test_limits_are_not_implemented_errors():
  with pytest.raises(NotImplementedError, match='n_pitches = 1$'):
    losses.HmmTranscriber(n_pitches=1)
  with pytest.raises(NotImplementedError, match='1024.*n_pitches = 1025'):
    losses.HmmTranscriber(n_pitches=1025)
  with pytest.raises(NotImplementedError, match='avg_length'):
    losses.HmmTranscriber(avg_length=1.0)
  with pytest.raises(NotImplementedError, match='avg_length'):
    losses.HmmTranscriber(avg_length=1.4, n_pitches=3)            # hold 0.286 < other 0.357
  losses.HmmTranscriber(avg_length=1.6, n_pitches=3)              # hold 0.375 >= other 0.3125
  losses.HmmTranscriber(n_pitches=2)
  losses.HmmTranscriber(n_pitches=1024)


def test_straight_through():
  x = torch.tensor([0.2, 1.7, 63.4], dtype=torch.float32, requires_grad=True)
  x_quant = torch.tensor([0.0, 2.0, 63.0], dtype=torch.float32)
  out = losses.HmmTranscriber.straight_through(x, x_quant)
  assert torch.allclose(out, x_quant, rtol=0.0, atol=1e-6)
  cot = torch.tensor([1.0, -2.0, 0.5])
  grad, = torch.autograd.grad(out, x, cot)
  assert torch.equal(grad, cot)
