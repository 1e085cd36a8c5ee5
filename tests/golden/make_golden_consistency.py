"""Generate tests/golden/consistency_*.npz by running the REFERENCE'S OWN losses.py / core.py on the numpy TensorFlow
stand-in of tf_numpy_shim.py (see make_golden.py).

    python tests/golden/make_golden_consistency.py        (needs the reference checkout; DDSP_REFERENCE_ROOT)

Ops this part of the reference calls and the stand-in lacks are supplied here at run time, among them a stand-in for
tensorflow_probability.distributions: Normal, Categorical(logits | probs=) and MixtureSameFamily.log_prob with TFP's
[sample, batch, event] broadcasting, in fp32 and in TFP's op order (Normal.log_prob takes x / scale - loc / scale;
MixtureSameFamily adds log_softmax of the mixture's logits and reduces with a max-subtracted log-sum-exp).

Every fixture is checked against the fp64 truth of tests/consistency_truth.py before it is written: one that the
reference's own fp32 result does not hold to REFUSE relative (of the tensor's largest value) is refused."""
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import tf_numpy_shim  # noqa: E402

if os.environ.get('DDSP_REFERENCE_ROOT'):
  tf_numpy_shim.install(os.environ['DDSP_REFERENCE_ROOT'])
else:
  tf_numpy_shim.install()
v2 = sys.modules['tensorflow.compat.v2']
_TENSOR = type(v2.linspace(0.0, 1.0, 2))
F32 = np.float32


def _t(x):
  return np.asarray(x, F32).view(_TENSOR)


def _logsumexp(x, axis=-1):
  x = np.asarray(x, F32)
  m = np.max(x, axis=axis, keepdims=True)
  m = np.where(np.isfinite(m), m, F32(0.0))
  with np.errstate(divide='ignore'):
    return (np.log(np.sum(np.exp(x - m), axis=axis, dtype=F32)) + np.squeeze(m, axis)).astype(F32)


class Normal:
  def __init__(self, loc, scale):
    self.loc, self.scale = np.asarray(loc, F32), np.asarray(scale, F32)

  def log_prob(self, x):
    x = np.asarray(x, F32)
    d = x / self.scale - self.loc / self.scale
    return F32(-0.5) * d * d - (F32(0.5 * math.log(2.0 * math.pi)) + np.log(self.scale))


class Categorical:
  def __init__(self, logits=None, probs=None):
    with np.errstate(divide='ignore'):
      self.logits = np.asarray(logits, F32) if logits is not None else np.log(np.asarray(probs, F32))

  def log_softmax(self):
    return self.logits - _logsumexp(self.logits)[..., None]


class MixtureSameFamily:
  def __init__(self, mixture_distribution, components_distribution):
    self.mix, self.comp = mixture_distribution, components_distribution

  def log_prob(self, x):
    lp = self.comp.log_prob(np.asarray(x, F32)[..., None])              # [sample, batch, components]
    return _t(_logsumexp(lp + self.mix.log_softmax(), axis=-1))


def _supply(module, name, fn):
  if not hasattr(module, name):
    setattr(module, name, fn)


tfp = sys.modules['tensorflow_probability']
for _cls in (Normal, Categorical, MixtureSameFamily):
  _supply(tfp.distributions, _cls.__name__, _cls)


def _softmax(x, axis=-1):
  x = np.asarray(x, F32)
  e = np.exp(x - x.max(axis=axis, keepdims=True))
  return _t(e / e.sum(axis=axis, keepdims=True, dtype=F32))


_supply(v2, 'ones', lambda shape, dtype=None: _t(np.ones(shape, F32)))
_supply(v2, 'ones_like', lambda x, dtype=None: _t(np.ones_like(np.asarray(x, F32))))
_supply(v2, 'zeros_like', lambda x, dtype=None: _t(np.zeros_like(np.asarray(x, F32))))
_supply(v2, 'range', lambda a, b=None, delta=1, dtype=None: _t(np.arange(a, b, delta)))
_supply(v2, 'transpose', lambda x, perm=None: _t(np.transpose(np.asarray(x), perm)))
_supply(v2, 'less_equal', lambda a, b: np.less_equal(np.asarray(a), b))
_supply(v2, 'maximum', lambda a, b: _t(np.maximum(np.asarray(a, F32), np.asarray(b, F32))))
_supply(v2.nn, 'softmax', _softmax)

from ddsp import core, losses  # noqa: E402  (the reference's files)
import consistency_truth as T  # noqa: E402
import torch  # noqa: E402

REFUSE = 5e-5 / 2.8    # the scalar ceiling of DESIGN.md section 2 over the room the Sinusoidal generator keeps (its ROOM)


def a(x):
  return np.ascontiguousarray(np.asarray(x, dtype=F32))


def _held(name, key, ref, truth):
  ref, truth = np.asarray(ref, np.float64), np.asarray(truth.numpy() if isinstance(truth, torch.Tensor) else truth, np.float64)
  scale = max(float(np.max(np.abs(truth))), 1e-30)
  err = float(np.max(np.abs(ref - truth))) / scale
  print('%-34s %-18s reference vs fp64 truth %.3e' % (name, key, err))
  assert err <= REFUSE, 'the reference itself is %.3e from the truth: not a usable fixture' % err


def save(name, **arrays):
  np.savez_compressed(os.path.join(HERE, name + '.npz'), **arrays)


def sinusoids(seed, b=2, t=12, k=8, zeros=False):
  rng = np.random.default_rng(seed)
  amps, freqs = T.make_sinusoids(rng, b, t, k, zeros=zeros)
  return rng, amps, freqs


def s2h_case(name, seed, normalize):
  rng, amps, freqs = sinusoids(seed)
  f0 = rng.uniform(150.0, 900.0, (2, 12, 1)).astype(F32)                 # 12 harmonics of 900 Hz pass 8 kHz
  freqs = (f0 * rng.integers(1, 12, freqs.shape) * rng.uniform(0.97, 1.03, freqs.shape)).astype(F32)
  kw = dict(harmonic_width=0.1, n_harmonics=12, sample_rate=16000, normalize=normalize)
  harm_amp, harm_dist = core.sinusoidal_to_harmonic(amps, freqs, f0, **kw)
  truth = T.sinusoidal_to_harmonic(amps, freqs, f0, **kw)
  _held(name, 'harm_amp', harm_amp, truth[0]); _held(name, 'harm_dist', harm_dist, truth[1])
  save(name, sin_amps=amps, sin_freqs=freqs, f0_hz=f0, normalize=int(normalize), harm_amp=a(harm_amp), harm_dist=a(harm_dist))


def twm_case(name, seed, own_candidates):
  rng, amps, freqs = sinusoids(seed)
  f0c = freqs if own_candidates else rng.uniform(100.0, 900.0, (2, 12, 1)).astype(F32)
  loss = losses.TWMLoss()
  s, h = loss.get_loss_tensors(f0c, freqs, amps)
  scalar = loss(f0c, freqs, amps)
  f0 = loss.predict_f0(f0c, freqs, amps)
  truth = T.twm_loss_tensors(f0c, freqs, amps)
  _held(name, 'sinusoids_loss', s, truth[0]); _held(name, 'harmonics_loss', h, truth[1])
  _held(name, 'scalar', scalar, T.twm_loss(f0c, freqs, amps))
  save(name, f0_candidates=f0c, freqs=freqs, amps=amps, sinusoids_loss=a(s), harmonics_loss=a(h), loss=a(scalar), f0_hz=a(f0))


def kde_case(name, seed, zeros, **kw):
  rng, amps_a, freqs_a = sinusoids(seed, zeros=zeros)
  amps_b, freqs_b = T.make_sinusoids(rng, 2, 12, 6)
  loss = losses.KDEConsistencyLoss(**kw)
  scalar = loss(amps_a, freqs_a, amps_b, freqs_b)
  nll = loss.nll(amps_a, freqs_a, amps_b, freqs_b, loss.scale_b)
  _held(name, 'nll', nll, T.kde_nll(amps_a, freqs_a, amps_b, freqs_b, loss.scale_b))
  _held(name, 'scalar', scalar, T.kde_loss(amps_a, freqs_a, amps_b, freqs_b, **kw))
  save(name, amps_a=amps_a, freqs_a=freqs_a, amps_b=amps_b, freqs_b=freqs_b, nll=a(nll), loss=a(scalar),
       **{k: np.float64(v) for k, v in kw.items()})


def thin_case(name, seed):
  rng = np.random.default_rng(seed)
  amp, amp_t = (rng.uniform(0.0, 3e-4, (2, 12, 1)).astype(F32) for _ in range(2))           # some targets under 1e-4
  dist, dist_t = (rng.uniform(0.0, 1.0, (2, 12, 8)).astype(F32) for _ in range(2))
  f0, f0_t = (rng.uniform(50.0, 900.0, (2, 12, 1)).astype(F32) for _ in range(2))
  out = losses.HarmonicConsistencyLoss()(amp, amp_t, dist, dist_t, f0, f0_t)
  truth = T.harmonic_consistency(amp, amp_t, dist, dist_t, f0, f0_t)
  for key in out:
    _held(name, key, out[key], truth[key])
  amp_log = losses.amp_loss(dist, dist_t, log=True)
  freq = losses.freq_loss(f0, f0_t)
  param = losses.ParamLoss(loss_type='L2')(dist, dist_t)
  _held(name, 'amp_loss_log', amp_log, T.amp_loss(dist, dist_t, log=True)); _held(name, 'freq_loss', freq, T.freq_loss(f0, f0_t))
  save(name, harm_amp=amp, harm_amp_target=amp_t, harm_dist=dist, harm_dist_target=dist_t, f0_hz=f0, f0_hz_target=f0_t,
       amp_loss_log=a(amp_log), freq_loss=a(freq), param_loss_l2=a(param), **{k: a(v) for k, v in out.items()})


if __name__ == '__main__':
  s2h_case('consistency_s2h', 1, False)
  s2h_case('consistency_s2h_normalize', 2, True)
  twm_case('consistency_twm_own_candidates', 3, True)
  twm_case('consistency_twm_c1', 4, False)
  kde_case('consistency_kde_default', 5, False)
  kde_case('consistency_kde_finetune', 8, False, weight_a=0.1, weight_b=0.1, weight_mean_amp=0.1, scale_a=0.1, scale_b=0.1)   # finetune_model.gin
  kde_case('consistency_kde_zero_frame', 6, True)
  thin_case('consistency_thin_losses', 7)
