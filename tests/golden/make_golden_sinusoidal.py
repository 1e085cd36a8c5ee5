"""Generate tests/golden/sinusoidal_*.npz by running the REFERENCE'S OWN core.py / synths.py on the numpy TensorFlow
stand-in of tf_numpy_shim.py (see make_golden.py).

    python tests/golden/make_golden_sinusoidal.py        (needs the reference checkout; DDSP_REFERENCE_ROOT)

Ops this part of the reference calls and the stand-in lacks are supplied here at run time, on the module the reference
imports (tensorflow.compat.v2).  The cumulative sum stays the sequential fp32 sum it is in TF.

Clips of at most 1600 samples and frequencies below 1.5 kHz: the reference's fp32 phase sum drifts with length and
frequency.  Every audio fixture is checked against the fp64 truth of tests/sinusoidal_truth.py (evaluated at the reference's
own fp32 controls) before it is written: one that the reference itself does not hold to 2e-3 / 2.8 (the room DESIGN.md
section 2 item 1 reports) is refused."""
import os
import sys

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


def _t(x):
  return np.asarray(x, np.float32).view(_TENSOR)


def _cumsum(x, axis=0, exclusive=False, reverse=False):
  assert not reverse and not exclusive
  x = np.asarray(x)
  return np.cumsum(x, axis=axis, dtype=x.dtype).view(_TENSOR)


def _softmax(x, axis=-1):
  x = np.asarray(x, np.float32)
  e = np.exp(x - x.max(axis=axis, keepdims=True))
  return _t(e / e.sum(axis=axis, keepdims=True, dtype=np.float32))


def _sigmoid(x):
  x = np.asarray(x, np.float32)
  return _t(np.float32(1.0) / (np.float32(1.0) + np.exp(-x)))


def _supply(module, name, fn):
  if not hasattr(module, name):
    setattr(module, name, fn)


v2.cumsum = _cumsum
v2.math.cumsum = _cumsum
_supply(v2.nn, 'softmax', _softmax)
_supply(v2.nn, 'sigmoid', _sigmoid)
_supply(v2, 'less_equal', lambda a, b: np.less_equal(np.asarray(a), b))
_supply(v2, 'equal', lambda a, b: np.equal(np.asarray(a), b))
_supply(v2, 'clip_by_value', lambda x, lo, hi: _t(np.clip(np.asarray(x), lo, hi)))
_supply(v2, 'stack', lambda xs, axis=0: _t(np.stack([np.asarray(x) for x in xs], axis=axis)))

from ddsp import core, synths  # noqa: E402  (the reference's files)
import sinusoidal_truth as T  # noqa: E402

GOLDEN_TOL = 2e-3
ROOM = 2.8


def a(x):
  return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def class_case(name, seed, B, F, K, N, kind, depth, amp_scale, method):
  rng = np.random.default_rng(seed)
  if kind == 'none':
    amps = rng.uniform(0.0, 1.0, (B, F, K)).astype(np.float32)
    freqs = np.exp(rng.uniform(np.log(40.0), np.log(1500.0), (B, F, K))).astype(np.float32)
    fn = None
  else:
    amps = rng.standard_normal((B, F, K)).astype(np.float32)
    # low network outputs: the scale functions then stay below ~1.5 kHz
    freqs = (rng.standard_normal((B, F, K * depth)) - (2.0 if kind == 'sigmoid' else 0.0)).astype(np.float32)
    ref_fn = core.frequencies_sigmoid if kind == 'sigmoid' else core.frequencies_softmax
    hz_max = 8000.0 if kind == 'sigmoid' else 1500.0
    fn = lambda x: ref_fn(x, depth=depth, hz_max=hz_max)  # noqa: E731
    assert kind == 'sigmoid' or hz_max == 1500.0
  synth = synths.Sinusoidal(n_samples=N, sample_rate=16000, amp_scale_fn=core.exp_sigmoid if amp_scale else None,
                            freq_scale_fn=fn, amp_resample_method=method)
  controls = synth.get_controls(amps, freqs)
  audio = a(synth.get_signal(**controls))
  truth = T.get_signal(a(controls['amplitudes']), a(controls['frequencies']), N, 16000, method)
  err = float(np.abs(audio.astype(np.float64) - truth).max())
  print('%-44s reference vs fp64 truth %.3e (max frequency %.0f Hz)' % (name, err, float(np.max(controls['frequencies']))))
  assert err <= GOLDEN_TOL / ROOM, 'the reference itself is %.3e from the truth: not a usable fixture' % err
  np.savez_compressed(os.path.join(HERE, name + '.npz'), amplitudes=amps, frequencies=freqs, n_samples=N, sample_rate=16000,
                      freq_fn=kind, depth=depth, hz_max=(8000.0 if kind != 'softmax' else 1500.0), amp_scale=int(amp_scale),
                      method=method, audio=audio)


def scale_function_case(name):
  rng = np.random.default_rng(21)
  arrays = {}
  for depth in (1, 8):
    x = (3.0 * rng.standard_normal((2, 7, 5 * depth))).astype(np.float32)
    arrays['x_d%d' % depth] = x
    arrays['sigmoid_d%d' % depth] = a(core.frequencies_sigmoid(x, depth=depth))
    arrays['softmax_d%d' % depth] = a(core.frequencies_softmax(x, depth=depth))
    for kind, fn in (('sigmoid', T.frequencies_sigmoid), ('softmax', T.frequencies_softmax)):
      rel = float(np.abs(arrays['%s_d%d' % (kind, depth)] / fn(x, depth) - 1.0).max())
      print('%-44s frequencies_%s depth %d: reference vs fp64 truth %.3e (relative)' % (name, kind, depth, rel))
      assert rel <= 2e-5 / ROOM
  harm_amp = rng.uniform(0.1, 1.0, (2, 9, 1)).astype(np.float32)
  harm_dist = rng.uniform(0.0, 1.0, (2, 9, 12)).astype(np.float32)
  f0_hz = rng.uniform(100.0, 1500.0, (2, 9, 1)).astype(np.float32)
  amps, freqs = core.harmonic_to_sinusoidal(harm_amp, harm_dist, f0_hz)
  np.savez_compressed(os.path.join(HERE, name + '.npz'), harm_amp=harm_amp, harm_dist=harm_dist, f0_hz=f0_hz, sin_amps=a(amps),
                      sin_freqs=a(freqs), **arrays)


if __name__ == '__main__':
  class_case('sinusoidal_class_default_f25_k8', 1, 2, 25, 8, 1600, 'sigmoid', 1, True, 'window')
  class_case('sinusoidal_class_softmax_d16_linear', 2, 2, 20, 5, 1600, 'softmax', 16, True, 'linear')
  class_case('sinusoidal_controls_f50_k6', 3, 2, 50, 6, 1600, 'none', 1, False, 'window')
  scale_function_case('sinusoidal_scale_functions')
