"""Generate tests/golden/fir_*.npz by running the REFERENCE'S OWN core.py (sinc_impulse_response, sinc_filter and
frequency_filter, ddsp/core.py:1568-1690) on the numpy TensorFlow stand-in of tf_numpy_shim.py.

    python tests/golden/make_golden_fir.py        (needs the reference checkout; DDSP_REFERENCE_ROOT)

The stand-in is set up by make_golden_consistency.py (imported, not run); the ops these functions call and the stand-in
lacks - tf.signal.hamming_window above all - are supplied here at run time, in fp32.  hamming_window follows TensorFlow's
_raised_cosine_window (window_ops.py) as the stand-in's hann_window does: a window of odd length, which is what
sinc_impulse_response always asks for, divides by length - 1 whether periodic or not.  Every fixture is checked against the
fp64 truth of tests/fir_truth.py before it is written.  The reference scales a numpy cutoff IN PLACE when a sample rate is
given (core.py:1598): it is handed a copy."""
import numpy as np

import make_golden_consistency as base            # installs the stand-in and imports the reference's core
import fir_truth as T  # noqa: E402

v2, core, F32 = base.v2, base.core, np.float32
REFUSE = 2e-6                                      # absolute, on unit-scale outputs and taps below 1


def _hamming_window(n, periodic=True, dtype=F32):
  n = int(n)
  if n == 1:
    return base._t(np.ones(1, F32))
  d = n + (1 if periodic else 0) * (1 - n % 2) - 1
  count = np.arange(n, dtype=F32)
  return base._t(F32(0.54) - F32(0.46) * np.cos(F32(2.0 * np.pi) * count / F32(d), dtype=F32))


def _range(start, limit=None, delta=1, dtype=None):
  if limit is None:
    start, limit = 0, start
  return base._t(np.arange(start, limit, delta, dtype=dtype or F32))


base._supply(v2.signal, 'hamming_window', _hamming_window)
for _name, _fn in (('range', _range), ('abs', lambda x: base._t(np.abs(np.asarray(x, F32)))),
                   ('sin', lambda x: base._t(np.sin(np.asarray(x, F32)))),
                   ('ones_like', lambda x: base._t(np.ones_like(np.asarray(x, F32)))),
                   ('convert_to_tensor', lambda x, dtype=None: base._t(np.asarray(x, F32))), ('newaxis', None)):
  base._supply(v2, _name, _fn)


def _held(name, key, ref, truth):
  err = float(np.max(np.abs(np.asarray(ref, np.float64) - truth.numpy())))
  print('%-30s %-8s reference vs fp64 truth %.3e' % (name, key, err))
  assert err <= REFUSE, 'the reference itself is %.3e from the truth: not a usable fixture' % err


def sinc_ir_case(name, seed, window_size):
  rng = np.random.default_rng(seed)
  cutoff = rng.uniform(0.05, 0.95, (2, 3, 1)).astype(F32)
  arrays = dict(cutoff=cutoff, window_size=np.int64(window_size))
  for hp in (0, 1):
    ref = np.asarray(core.sinc_impulse_response(cutoff.copy(), window_size=window_size, high_pass=bool(hp)), F32)
    _held(name, 'ir_hp%d' % hp, ref, T.sinc_impulse_response(cutoff, window_size, None, bool(hp)))
    arrays['ir_hp%d' % hp] = base.a(ref)
  base.save(name, **arrays)


def sinc_filter_case(name, seed, window_size, sample_rate):
  rng = np.random.default_rng(seed)
  audio = rng.uniform(-1.0, 1.0, (2, 240)).astype(F32)
  cutoff = rng.uniform(0.05, 0.95, (2, 4, 1)).astype(F32) * F32(sample_rate / 2.0)
  ref = np.asarray(core.sinc_filter(audio, cutoff.copy(), window_size=window_size, sample_rate=sample_rate), F32)
  _held(name, 'out', ref, T.sinc_filter(audio, cutoff, window_size, sample_rate))
  base.save(name, audio=audio, cutoff=cutoff, window_size=np.int64(window_size), sample_rate=np.int64(sample_rate), out=base.a(ref))


def frequency_filter_case(name, seed, window_size):
  rng = np.random.default_rng(seed)
  audio = rng.uniform(-1.0, 1.0, (2, 240)).astype(F32)
  mags = rng.uniform(0.0, 1.0, (2, 4, 33)).astype(F32)
  ref = np.asarray(core.frequency_filter(audio, mags, window_size=window_size), F32)
  _held(name, 'out', ref, T.frequency_filter(audio, mags, window_size))
  base.save(name, audio=audio, magnitudes=mags, window_size=np.int64(window_size), out=base.a(ref))


if __name__ == '__main__':
  sinc_ir_case('fir_sinc_impulse_response', 31, 64)
  sinc_filter_case('fir_sinc_filter', 32, 64, 16000)
  frequency_filter_case('fir_frequency_filter', 33, 33)
