"""Generate tests/golden/core_rest_*.npz by running the REFERENCE'S OWN core.py on the numpy TensorFlow stand-in of
tf_numpy_shim.py (see make_golden.py): frequencies_critical_bands, harmonic_distribution_to_wavetable and the elementwise
scale functions.

    python tests/golden/make_golden_core_rest.py        (needs the reference checkout; DDSP_REFERENCE_ROOT)

Ops this part of the reference calls and the stand-in lacks (tanh, softplus, range) are supplied here at run time, on the
module the reference imports (tensorflow.compat.v2).  TensorFlow turns the numpy float64 tables of
frequencies_critical_bands into fp32 tensors where they meet the network outputs; numpy would promote the product to
float64 instead, so the supplied softplus takes its argument as fp32, which is where the reference's chain is fp32 again.

The cases and their inputs are those of tests/test_gpu_core_rest.py (imported from there: one definition).  Before a
fixture is written the reference's output is checked against the fp64 truth of tests/core_rest_truth.py at the tolerance
the kernels are held to: a fixture the reference itself does not hold is refused."""
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


def _softplus(x):
  x = np.asarray(x).astype(np.float32)
  return _t(np.maximum(x, np.float32(0.0)) + np.log1p(np.exp(-np.abs(x))))


def _supply(module, name, fn):
  if not hasattr(module, name):
    setattr(module, name, fn)


_supply(v2.nn, 'tanh', lambda x: _t(np.tanh(np.asarray(x, np.float32))))
_supply(v2.nn, 'softplus', _softplus)
_supply(v2, 'range', lambda *args, dtype=np.float32: _t(np.arange(*args).astype(dtype)))

from ddsp import core  # noqa: E402  (the reference's file)
import core_rest_truth as T  # noqa: E402
import core_rest_cases as C  # noqa: E402


def a(x):
  return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def critical_bands():
  arrays = {}
  for name in C.CRITICAL_BAND_GOLDEN_CASES:
    k = C.CRITICAL_BAND_CASES[name][0]
    kwargs = C.critical_band_kwargs(name)
    x = C.critical_band_input(name)
    out = a(core.frequencies_critical_bands(_t(x), **kwargs))
    truth = T.critical_bands(x, k, **kwargs)
    tol = T.critical_bands_tolerance(k, **kwargs)
    err = float(np.abs(out - truth).max())
    print('critical bands %-24s reference vs fp64 truth %.3e (tolerance %.3e)' % (name, err, tol))
    assert out.shape == truth.shape and err <= tol, 'the reference itself misses the tolerance: not a usable fixture'
    arrays[name + '/x'], arrays[name + '/out'] = x, out
    for key, value in kwargs.items():
      arrays[name + '/' + key] = np.asarray(value)
  np.savez_compressed(os.path.join(HERE, 'core_rest_critical_bands.npz'), **arrays)


def wavetables():
  arrays = {}
  for name in C.WAVETABLE_GOLDEN_CASES:
    k, n_wavetable, _ = C.WAVETABLE_CASES[name]
    hd = C.wavetable_input(name)
    out = a(core.harmonic_distribution_to_wavetable(_t(hd), n_wavetable=n_wavetable))
    truth = T.wavetable(hd, n_wavetable)
    tol = T.wavetable_tolerance(truth, k, n_wavetable)
    err = float(np.abs(out - truth).max())
    print('wavetable %-24s reference vs fp64 truth %.3e (tolerance %.3e)' % (name, err, tol))
    assert out.shape == truth.shape and err <= tol, 'the reference itself misses the tolerance: not a usable fixture'
    arrays[name + '/harmonic_distribution'], arrays[name + '/out'], arrays[name + '/n_wavetable'] = hd, out, np.asarray(n_wavetable)
  np.savez_compressed(os.path.join(HERE, 'core_rest_wavetable.npz'), **arrays)


def elementwise():
  arrays = {}
  for name, (fn_name, kwargs, _) in C.ELEMENTWISE_CASES.items():
    x = C.elementwise_input(name)
    with np.errstate(divide='ignore', invalid='ignore'):
      out = a(getattr(core, fn_name)(_t(x), **kwargs))
    truth = getattr(T, fn_name)(x, **kwargs)
    tol = T.elementwise_tolerance(truth)
    err = np.abs(out - truth)
    print('elementwise %-24s reference vs fp64 truth %.3e of the tolerance' % (name, float(np.max(err / tol))))
    assert out.shape == truth.shape and np.all(err <= tol), 'the reference itself misses the tolerance: not a usable fixture'
    arrays[name + '/x'], arrays[name + '/out'], arrays[name + '/function'] = x, out, np.asarray(fn_name)
    for key, value in kwargs.items():
      arrays[name + '/' + key] = np.asarray(value)
  np.savez_compressed(os.path.join(HERE, 'core_rest_elementwise.npz'), **arrays)


if __name__ == '__main__':
  critical_bands()
  wavetables()
  elementwise()
