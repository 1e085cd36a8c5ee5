"""Generate tests/golden/wavetable_*.npz, variable_length_delay_*.npz and mod_delay_*.npz by running the REFERENCE'S
OWN core.py / synths.py / effects.py on the numpy TensorFlow stand-in of tf_numpy_shim.py (see make_golden.py).

    python tests/golden/make_golden_wavetable.py        (needs the reference checkout; DDSP_REFERENCE_ROOT)

The stand-in lacks two ops this part of the reference calls, tf.nn.relu and tf.cumsum(exclusive=True); both are supplied
here at run time, on the module the reference imports (tensorflow.compat.v2).  The cumulative sum stays the sequential
fp32 sum it is in TF.

The synthesis fixtures use SMOOTH (8-harmonic) tables and clips of at most 1600 samples: the reference's fp32 phase error
times the table's slope is what separates it from the truth, and with white tables that is 1e-2 and more.  Every
fixture is checked against the fp64 truth of tests/wavetable_truth.py before it is written: one that the reference
itself does not hold to 2e-3 / 2.8 (the room DESIGN.md section 2 item 1 reports) is refused."""
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
  tf_numpy_shim.install()                                 # the stand-in's own default location of the reference checkout
v2 = sys.modules['tensorflow.compat.v2']
_TENSOR = type(v2.linspace(0.0, 1.0, 2))


def _relu(x):
  x = np.asarray(x)
  return np.maximum(x, x.dtype.type(0)).view(_TENSOR)


def _cumsum(x, axis=0, exclusive=False, reverse=False):
  assert not reverse
  x = np.asarray(x)
  total = np.cumsum(x, axis=axis, dtype=x.dtype)
  if exclusive:                                            # shifted by one: [0, x0, x0 + x1, ...]
    total = np.concatenate([np.zeros_like(np.take(total, [0], axis=axis)),
                            np.take(total, np.arange(x.shape[axis] - 1), axis=axis)], axis=axis)
  return total.view(_TENSOR)


v2.nn.relu = _relu
v2.cumsum = _cumsum
v2.math.cumsum = _cumsum

from ddsp import core, effects, synths  # noqa: E402  (the reference's files)
import wavetable_truth as T  # noqa: E402

GOLDEN_TOL = 2e-3
ROOM = 2.8


def a(x):
  return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def save(name, truth, key, **arrays):
  err = float(np.abs(np.asarray(arrays[key], np.float64) - truth).max())
  print('%-40s reference vs fp64 truth %.3e' % (name, err))
  assert err <= GOLDEN_TOL / ROOM, 'the reference itself is %.3e from the truth: not a usable fixture' % err
  np.savez_compressed(os.path.join(HERE, name + '.npz'), **arrays)


def synthesis_inputs(seed, B, F, W, Fw, scaled):
  rng = np.random.default_rng(seed)
  tables = T.smooth_tables(rng, B, Fw, W)
  amps = rng.uniform(0.1, 1.0, (B, F, 1)).astype(np.float32)
  if scaled:                                               # raw network outputs; exp_sigmoid keeps smooth tables smooth
    amps = rng.standard_normal((B, F, 1)).astype(np.float32)
    tables = (2.0 * tables).astype(np.float32)
  f0 = np.exp(rng.uniform(np.log(60.0), np.log(1200.0), (B, F, 1))).astype(np.float32)
  return amps, tables, f0


def class_case(name, seed, B, F, W, N, scaled):
  amps, tables, f0 = synthesis_inputs(seed, B, F, W, F, scaled)
  synth = synths.Wavetable(n_samples=N, sample_rate=16000, scale_fn=core.exp_sigmoid if scaled else None)
  audio = a(synth(amps, tables, f0))
  truth = T.wavetable_synthesis(f0, amps, tables, N, 16000, scale=scaled)
  save(name, truth, 'audio', amplitudes=amps, wavetables=tables, f0_hz=f0, n_samples=N, sample_rate=16000, scaled=int(scaled),
       audio=audio)


def synthesis_case(name, seed, B, F, W, N, Fw):
  amps, tables, f0 = synthesis_inputs(seed, B, F, W, Fw, False)
  if Fw == 1:
    tables = tables[:, 0]
  audio = a(core.wavetable_synthesis(f0, amps, tables, N, 16000))
  truth = T.wavetable_synthesis(f0, amps, tables, N, 16000)
  save(name, truth, 'audio', amplitudes=amps, wavetables=tables, f0_hz=f0, n_samples=N, sample_rate=16000, audio=audio)


def delay_case(name, seed, B, N, L):
  rng = np.random.default_rng(seed)
  audio = T.smooth_tables(rng, B, 1, N, 20)[:, 0]
  phase = rng.uniform(0.0, 1.0, (B, N, 1)).astype(np.float32)
  out = a(core.variable_length_delay(phase, audio, L))
  truth = T.variable_length_delay(phase[..., 0], audio, L)
  save(name, truth, 'out', phase=phase, audio=audio, max_length=L, out=out, scaled=0, gain_max=1.0)


def mod_delay_case(name, seed, B, N, add_dry, scaled):
  rng = np.random.default_rng(seed)
  audio = T.smooth_tables(rng, B, 1, N, 20)[:, 0]
  gain = rng.standard_normal((B, N, 1)).astype(np.float32)
  phase = (rng.standard_normal((B, N, 1)) if scaled else rng.uniform(-1, 1, (B, N, 1))).astype(np.float32)
  kw = {} if scaled else dict(gain_scale_fn=None, phase_scale_fn=None)
  fx = effects.ModDelay(add_dry=add_dry, **kw)
  out = a(fx(audio, gain, phase))
  truth = T.mod_delay(audio, gain[..., 0], phase[..., 0], add_dry=add_dry, scale=scaled)
  gain_max = float(np.abs(T.exp_sigmoid(gain) if scaled else gain).max())
  save(name, truth, 'out', audio=audio, gain=gain, phase=phase, add_dry=int(add_dry), scaled=int(scaled), out=out,
       max_length=int(16000 / 1000.0 * 25.0), gain_max=gain_max)


if __name__ == '__main__':
  class_case('wavetable_class_f25_w2048', 1, 2, 25, 2048, 1600, False)
  class_case('wavetable_class_scaled_f25_w256', 2, 2, 25, 256, 1600, True)
  synthesis_case('wavetable_synthesis_static_w1024', 3, 2, 25, 1024, 1600, 1)
  synthesis_case('wavetable_synthesis_frames50_vs_25', 4, 2, 25, 512, 1600, 50)
  delay_case('variable_length_delay_l400', 5, 2, 1200, 400)
  mod_delay_case('mod_delay_default', 6, 2, 1200, True, True)
  mod_delay_case('mod_delay_no_dry_no_scale', 7, 2, 1200, False, False)
