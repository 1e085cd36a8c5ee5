"""CPU tests of synths.Sinusoidal's host layer: the reference's signatures and defaults, its ValueErrors, the routing between
the closed-form kernels and the chain of materialised envelopes, the C ABI's argument checks, and the fp64 truth helper
(tests/sinusoidal_truth.py) against the oracle's composition, central differences and the reference's goldens."""
import functools
import inspect

import numpy as np
import pytest

import oracle.ddsp_oracle as O
import sinusoidal_truth as T
from conftest import load_golden
from ddsp_amd import _lib, core, synths
from ddsp_amd import build as build_mod


def defaults(fn):
  return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n != 'self']


def test_signatures_and_defaults_are_the_references():
  assert defaults(synths.Sinusoidal.__init__) == [
      ('n_samples', 64000), ('sample_rate', 16000), ('amp_scale_fn', core.exp_sigmoid), ('amp_resample_method', 'window'),
      ('freq_scale_fn', core.frequencies_sigmoid), ('name', 'sinusoidal')]
  assert [n for n, _ in defaults(synths.Sinusoidal.get_controls)] == ['amplitudes', 'frequencies']
  assert [n for n, _ in defaults(synths.Sinusoidal.get_signal)] == ['amplitudes', 'frequencies']
  E = inspect.Parameter.empty
  assert defaults(core.frequencies_sigmoid) == [('freqs', E), ('depth', 1), ('hz_min', 0.0), ('hz_max', 8000.0)]
  assert defaults(core.frequencies_softmax) == [('freqs', E), ('depth', 1), ('hz_min', 20.0), ('hz_max', 8000.0)]
  assert defaults(core.logb) == [('x', E), ('base', 2.0), ('eps', 1e-5)]
  assert defaults(core.midi_to_hz) == [('notes', E), ('midi_zero_silence', False)]
  assert defaults(core.hz_to_midi) == [('frequencies', E)]
  assert defaults(core.unit_to_midi) == [('unit', E), ('midi_min', 20.0), ('midi_max', 90.0), ('clip', False)]
  assert defaults(core.midi_to_unit) == [('midi', E), ('midi_min', 20.0), ('midi_max', 90.0), ('clip', False)]
  assert defaults(core.unit_to_hz) == [('unit', E), ('hz_min', E), ('hz_max', E), ('clip', False)]
  assert defaults(core.hz_to_unit) == [('hz', E), ('hz_min', E), ('hz_max', E), ('clip', False)]
  assert defaults(core.harmonic_to_sinusoidal) == [('harm_amp', E), ('harm_dist', E), ('f0_hz', E), ('sample_rate', 16000)]
  assert synths.Sinusoidal().name == 'sinusoidal'


def test_scale_functions_the_class_sees_through():
  assert synths.Sinusoidal()._freq_spec() == (_lib.SIN_FREQ_SIGMOID, 1, 0.0, 8000.0)
  shipped = synths.Sinusoidal(freq_scale_fn=functools.partial(core.frequencies_softmax, depth=64))
  assert shipped._freq_spec() == (_lib.SIN_FREQ_SOFTMAX, 64, 20.0, 8000.0)
  assert synths.Sinusoidal(freq_scale_fn=None)._freq_spec() == (0, 1, 0.0, 0.0)
  assert synths.Sinusoidal(freq_scale_fn=lambda x: core.frequencies_sigmoid(x, depth=10))._freq_spec() is None
  assert synths.Sinusoidal(freq_scale_fn=functools.partial(core.frequencies_sigmoid, depth=65))._freq_spec() is None
  assert synths.Sinusoidal(freq_scale_fn=functools.partial(core.frequencies_sigmoid, None))._freq_spec() is None


def test_routing_between_the_closed_form_kernels_and_the_chain():
  s = synths.Sinusoidal(n_samples=64000)
  assert s._on_fused_kernels((32, 1000, 100), (32, 1000, 100))
  assert s._on_fused_kernels((32, 1000, 100), (32, 1000, 6400), depth=64)
  assert not s._on_fused_kernels((32, 1000, 100), (32, 500, 100))                    # two frame grids
  assert not synths.Sinusoidal(n_samples=64001, amp_resample_method='linear')._on_fused_kernels((2, 1000, 10), (2, 1000, 10))
  assert synths.Sinusoidal(n_samples=64000, amp_resample_method='linear')._on_fused_kernels((2, 1000, 10), (2, 1000, 10))
  for method in ('nearest', 'cubic'):
    assert not synths.Sinusoidal(n_samples=64000, amp_resample_method=method)._on_fused_kernels((2, 1000, 10), (2, 1000, 10))


def test_value_errors_are_the_references():
  import torch
  a = torch.zeros((2, 10, 3))
  with pytest.raises(ValueError, match='is invalid'):
    core._check_amp_method('bogus', 10, 100)
  with pytest.raises(ValueError, match='divisible'):
    synths.Sinusoidal(n_samples=105)._synthesize.__func__          # (bound below: the check runs before any kernel)
    core._check_amp_method(synths.Sinusoidal(n_samples=105).amp_resample_method, 10, 105)
  with pytest.raises(ValueError, match='multiple of depth'):
    core._depth_layout(torch.zeros((2, 10, 7)), 2)
  with pytest.raises(ValueError, match='n_sinusoids'):
    core._depth_layout(torch.zeros((2, 10)), 1)
  with pytest.raises(ValueError, match='n_sinusoids'):
    synths.Sinusoidal._check_3d(a, a[0])
  flat, k, depth = core._depth_layout(torch.zeros((2, 10, 3, 4)), 1)
  assert tuple(flat.shape) == (2, 10, 12) and (k, depth) == (3, 4)


@pytest.fixture(scope='module')
def lib():
  build_mod.build()
  return _lib.load()


def test_c_abi_argument_checks(lib):
  names = [lib.ddsp_profile_kernel_name(i).decode() for i in range(lib.ddsp_profile_kernel_count())]
  assert 'sin_synth_kernel' in names and 'sin_bwd_sums_kernel' in names
  assert lib.ddsp_sinusoidal_workspace_bytes(32, 1000, 100, 64000) == 3 * 32 * 1000 * 100 * 4
  assert lib.ddsp_sinusoidal_backward_workspace_bytes(8, 1000, 100, 64000) == 10 * 8 * 1000 * 100 * 4
  assert lib.ddsp_sinusoidal_workspace_bytes(0, 1, 1, 1) == 0
  assert lib.ddsp_sinusoidal_signal_f32(None, None, None, None, 0, 1, 1, 1, 1, 16000.0, 0, None) == -1
  assert lib.ddsp_sinusoidal_signal_f32(16, 16, 16, 16, 0, 1, 3, 1, 10, 16000.0, 0, None) == _lib.ERR_UNSUPPORTED     # ragged
  assert lib.ddsp_sinusoidal_signal_f32(16, 16, 16, 16, 0, 1, 2, 1, 10, 16000.0, _lib.SIN_FREQ_SIGMOID, None) == _lib.ERR_UNSUPPORTED
  assert lib.ddsp_sinusoidal_signal_f32(16, 16, 16, 16, 0, 1, 2, 1, 10, 16000.0, 0, None) == -4                       # workspace
  assert lib.ddsp_sinusoidal_signal_f32(16, 16, 16, 16, 0, 0, 2, 1, 10, 16000.0, 0, None) == -2
  both = _lib.SIN_FREQ_SIGMOID | _lib.SIN_FREQ_SOFTMAX
  assert lib.ddsp_sinusoidal_controls_f32(None, 16, None, 16, 4, 2, 1, 0.0, 8000.0, 16000.0, both, None) == _lib.ERR_UNSUPPORTED
  assert lib.ddsp_sinusoidal_controls_f32(None, 16, None, 16, 4, 2, 65, 0.0, 8000.0, 16000.0, _lib.SIN_FREQ_SIGMOID, None) == \
      _lib.ERR_UNSUPPORTED
  assert lib.ddsp_sinusoidal_controls_f32(16, 16, None, 16, 4, 2, 1, 0.0, 8000.0, 16000.0, 0, None) == -1
  assert lib.ddsp_unit_convert_f32(16, 16, 4, 99, 0.0, 0.0, None) == _lib.ERR_UNSUPPORTED
  assert lib.ddsp_unit_convert_f32(None, 16, 4, 0, 0.0, 0.0, None) == -1


# ---- the truth helper --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method,N,F,tol', [('window', 1600, 25, 1e-8), ('linear', 640, 20, 1e-8), ('window', 4096, 2, 1e-8),
                                            ('linear', 300, 1, 1e-8), ('linear', 740, 20, 1e-4)])
def test_truth_equals_the_oracles_composition_in_fp64(method, N, F, tol):
  # (hop 37: the legacy resize takes its positions as t * fl32(F / N) in fp32, 1e-7 off r / hop; with power-of-two hops both
  #  are exact.  The closed forms use r / hop, as every synth kernel of this package does.)
  amps, freqs = T.control_inputs(N, 2, F, 5, f_hi=7990.0)
  freqs[0, F // 2, 0] = 9000.0                                         # one oscillator crosses Nyquist and comes back
  want = O.oscillator_bank(O.resample(freqs, N, dtype=np.float64), O.resample(amps, N, method, dtype=np.float64), 16000)
  assert np.abs(T.get_signal(amps, freqs, N, 16000, method) - want).max() < tol


@pytest.mark.parametrize('method,N,F', [('window', 320, 5), ('linear', 111, 3), ('linear', 64, 1)])
def test_truth_gradients_equal_central_differences(method, N, F):
  rng = np.random.default_rng(N)
  amps, freqs = T.control_inputs(N + 1, 1, F, 3, f_hi=3000.0)
  amps, freqs = amps.astype(np.float64), freqs.astype(np.float64)
  g = rng.standard_normal((1, N))
  ga, gf = T.get_signal_backward(amps, freqs, g, N, 16000, method)

  def loss(a, f):
    return float((T.get_signal(a, f, N, 16000, method) * g).sum())

  for grad, which, eps in ((ga, 0, 1e-6), (gf, 1, 1e-4)):
    for idx in np.ndindex(amps.shape):
      lo, hi = [amps.copy(), freqs.copy()], [amps.copy(), freqs.copy()]
      lo[which][idx] -= eps
      hi[which][idx] += eps
      fd = (loss(*hi) - loss(*lo)) / (2 * eps)
      assert abs(fd - grad[idx]) <= 1e-5 * np.abs(grad).max() + 1e-9, (which, idx, fd, grad[idx])


@pytest.mark.parametrize('kind,depth', [('sigmoid', 1), ('sigmoid', 5), ('softmax', 1), ('softmax', 6)])
def test_truth_scale_function_gradients_equal_central_differences(kind, depth):
  fn = T.frequencies_sigmoid if kind == 'sigmoid' else T.frequencies_softmax
  x = np.random.default_rng(depth).standard_normal((1, 2, 3 * depth))
  hz, dx = fn(x, depth, grad=True)
  eps = 1e-6
  for idx in np.ndindex(x.shape):
    lo, hi = x.copy(), x.copy()
    lo[idx] -= eps
    hi[idx] += eps
    fd = (fn(hi, depth) - fn(lo, depth)) / (2 * eps)
    k, i = divmod(idx[2], depth)
    assert abs(fd[idx[0], idx[1], k] - dx[idx[0], idx[1], k, i]) <= 1e-6 * np.abs(dx).max() + 1e-9
  assert np.all(T.frequencies_sigmoid(np.full((1, 1, 10), 50.0), 10) <= 8000.0 * (1 + 1e-12))
  assert sum(hi for _, hi in T.sigmoid_ranges(7, 0.0, 8000.0)) == pytest.approx(8000.0)


def test_truth_vs_the_references_goldens():
  for name in ('sinusoidal_class_default_f25_k8', 'sinusoidal_class_softmax_d16_linear', 'sinusoidal_controls_f50_k6'):
    z = load_golden(name)
    kind, depth = str(z['freq_fn']), int(z['depth'])
    fn = None if kind == 'none' else functools.partial(T.frequencies_sigmoid if kind == 'sigmoid' else T.frequencies_softmax,
                                                       depth=depth, hz_max=float(z['hz_max']))
    out = T.sinusoidal(z['amplitudes'], z['frequencies'], int(z['n_samples']), int(z['sample_rate']), str(z['method']),
                       bool(z['amp_scale']), fn)
    assert np.abs(out - z['audio']).max() <= 2e-3, name
  z = load_golden('sinusoidal_scale_functions')
  for depth in (1, 8):
    assert np.abs(T.frequencies_sigmoid(z['x_d%d' % depth], depth) / z['sigmoid_d%d' % depth] - 1).max() < 2e-5
    assert np.abs(T.frequencies_softmax(z['x_d%d' % depth], depth) / z['softmax_d%d' % depth] - 1).max() < 2e-5
  amps, freqs = T.harmonic_to_sinusoidal(z['harm_amp'], z['harm_dist'], z['f0_hz'])
  assert np.abs(amps - z['sin_amps']).max() < 2e-6 and np.abs(freqs / z['sin_freqs'] - 1).max() < 1e-6
