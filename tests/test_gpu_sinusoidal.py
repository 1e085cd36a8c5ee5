"""synths.Sinusoidal, core.frequencies_sigmoid / frequencies_softmax, the unit conversions and core.harmonic_to_sinusoidal on
the MI355X, forward and backward, against the fp64 truth of tests/sinusoidal_truth.py, the reference's own fp32 chain
(tests/golden/sinusoidal_*.npz, written by tests/golden/make_golden_sinusoidal.py) and the reference's unit tests,
re-expressed (ddsp/synths_test.py:73-110, core_test.py:27-140).

Tolerances.
  * audio against fp64 truth: C_FWD max(1, max_n sum_k a[n, k]), C_FWD = 6e-5, the figure the direct-sum Harmonic is held to
    (item 1).  The truth is evaluated at the fp32 CONTROLS.  Where the inputs are raw network outputs, the kernel's own
    controls are read back (return_outputs_dict) and held to the truth's controls on their own, relative to the value:
    C_CTL = 4e-6 for frequencies (exp2 / exp / the softmax sum in fp32, a few ulp) and amplitudes (exp_sigmoid on the
    hardware exp / log, the figure of test_gpu_wavetable.py).  The split is deliberate: one fp32 ulp of a 4 kHz frequency,
    held for 4 s, is 1e-3 cycles of phase, which no fp32 interface can avoid and which says nothing about the synthesis.
  * goldens: 2e-3 (item 1).
  * gradients: C_GRAD = 2e-4 of the largest truth gradient (item 5), at incoming gradients of 1e-6, 1 and 1e+6.
  * determinism: equal bits (item 4).
tests/test_sinusoidal_emulated.py runs the small cases of this file on the CPU emulation of the kernels."""
import functools

import numpy as np
import pytest
import torch

import sinusoidal_truth as T
from conftest import load_golden, parity_check

pytestmark = pytest.mark.gpu

DEV = 'cuda'
C_FWD = 6e-5
C_CTL = 4e-6
C_GRAD = 2e-4
GOLDEN_TOL = 2e-3


@pytest.fixture(scope='module')
def ddsp():
  if DEV == 'cuda':
    if not torch.cuda.is_available():
      pytest.skip('gpu tests need a GPU (run with -m gpu on an MI355X)')
    from ddsp_amd import build
    build.build()
  import ddsp_amd
  return ddsp_amd


def dev(x, grad=False):
  t = torch.as_tensor(np.asarray(x, np.float32), device=DEV)
  return t.requires_grad_(True) if grad else t


def npy(t):
  return t.detach().cpu().numpy()


def fwd_tol(amps, freqs, n, sr, method='window'):
  return C_FWD * max(1.0, T.amplitude_sum(amps, freqs, n, sr, method))


def controls_synth(ddsp, n, sr=16000, method='window'):
  return ddsp.synths.Sinusoidal(n_samples=n, sample_rate=sr, amp_scale_fn=None, freq_scale_fn=None, amp_resample_method=method)


# ---- 1. the reference's unit tests --------------------------------------------------------------------------------------
def test_synths_sinusoidal_output_shape_is_correct(ddsp):             # synths_test.py:75-87
  synth = ddsp.synths.Sinusoidal(n_samples=32000, sample_rate=16000)
  out = synth(torch.zeros((3, 1000, 10), device=DEV), torch.zeros((3, 1000, 10), device=DEV))
  assert list(out.shape) == [3, 32000]
  assert np.isfinite(npy(out)).all()


def test_synths_sinusoidal_frequencies_controls_are_bounded(ddsp):    # synths_test.py:89-110
  depth = 10

  def freq_scale_fn(x):
    return ddsp.core.frequencies_sigmoid(x, depth=depth, hz_min=0.0, hz_max=8000.0)

  synth = ddsp.synths.Sinusoidal(n_samples=32000, sample_rate=16000, freq_scale_fn=freq_scale_fn)
  freqs = np.tile(np.linspace(-100.0, 100.0, 100, dtype=np.float32)[None, None, :, None], [3, 10, 1, depth])
  controls = synth.get_controls(torch.zeros((3, 10, 100), device=DEV), dev(freqs))
  f = npy(controls['frequencies'])
  assert f.shape == (3, 10, 100)
  assert np.all((f <= 8000.0) & (f >= 0.0))


def test_core_midi_hz_conversions_are_accurate(ddsp):                 # core_test.py:27-40 (librosa's formulas, restated)
  midi = np.arange(128, dtype=np.float32)
  np.testing.assert_allclose(npy(ddsp.core.midi_to_hz(dev(midi))), 440.0 * 2.0 ** ((midi - 69.0) / 12.0), rtol=1e-6)
  hz = np.linspace(0.0, 20000.0, 128).astype(np.float32)
  np.testing.assert_allclose(npy(ddsp.core.hz_to_midi(dev(hz))), T.hz_to_midi(hz), rtol=1e-6, atol=1e-5)
  assert npy(ddsp.core.hz_to_midi(dev([0.0, -3.0]))).tolist() == [0.0, 0.0]
  assert npy(ddsp.core.midi_to_hz(dev([0.0, 69.0]), midi_zero_silence=True)).tolist() == [0.0, 440.0]
  x = np.array([8.0, 0.0, -1.0, 1e-3], np.float32)
  np.testing.assert_allclose(npy(ddsp.core.logb(dev(x))), T.logb(x), rtol=1e-6)
  np.testing.assert_allclose(npy(ddsp.core.logb(dev(x), base=10.0)), T.logb(x, 10.0), rtol=1e-6)


@pytest.mark.parametrize('clip', [True, False])
def test_core_midi_unit_conversions_are_accurate(ddsp, clip):          # core_test.py:42-74
  midi = np.linspace(0.0, 127.0, 1000).astype(np.float32)
  np.testing.assert_allclose(npy(ddsp.core.midi_to_unit(dev(midi), 20.0, 90.0, clip)), T.midi_to_unit(midi, 20.0, 90.0, clip),
                             rtol=1e-6, atol=1e-6)
  unit = np.linspace(-1.0, 2.0, 1000).astype(np.float32)
  np.testing.assert_allclose(npy(ddsp.core.unit_to_midi(dev(unit), 20.0, 90.0, clip)), T.unit_to_midi(unit, 20.0, 90.0, clip),
                             rtol=1e-6, atol=1e-5)


def test_core_unit_hz_conversions_are_accurate(ddsp):                 # core_test.py:76-92
  unit = np.linspace(0.0, 1.0, 128).astype(np.float32)
  hz = np.logspace(np.log10(20.0), np.log10(1000.0), 128)
  np.testing.assert_allclose(npy(ddsp.core.unit_to_hz(dev(unit), 20.0, 1000.0)), hz, rtol=1e-5)
  np.testing.assert_allclose(npy(ddsp.core.hz_to_unit(dev(hz), 20.0, 1000.0)), unit, rtol=1e-5, atol=1e-6)


def test_core_harmonic_to_sinusoidal(ddsp):                           # core_test.py:94-140
  f0 = npy(ddsp.core.midi_to_hz(dev([80, 81, 82, 81, 80])))[None, :, None]
  harm = np.ones((1, 5, 3)) / 3.0
  amps, freqs = ddsp.core.harmonic_to_sinusoidal(10, dev(harm), dev(f0))
  np.testing.assert_allclose(npy(amps), harm * 10, rtol=1e-6)
  np.testing.assert_allclose(npy(freqs), f0 * np.arange(1, 4), rtol=1e-6)
  f0 = np.asarray([200, 400, 8001], np.float32)[None, :, None]
  amps, freqs = ddsp.core.harmonic_to_sinusoidal(10, dev(np.ones((1, 3, 3)) / 3.0), dev(f0))
  expected = np.full((1, 3), 10.0 / 3.0)
  expected[:, 2] = 0
  np.testing.assert_allclose(npy(amps)[..., 0], expected, rtol=1e-6)
  np.testing.assert_allclose(npy(freqs), f0 * np.arange(1, 4), rtol=1e-6)
  f0 = np.asarray([50, 3001, 4001, 3001, 50], np.float32)[None, :, None]
  amps, _ = ddsp.core.harmonic_to_sinusoidal(10, dev(np.ones((1, 5, 3)) / 3.0), dev(f0))
  expected = np.ones((1, 5, 3)) * 10
  expected[:, 2, 1] = 0
  expected[:, 1:4, 2] = 0
  expected[:, 0] /= 3
  expected[:, 1] /= 2
  expected[:, 3] /= 2
  expected[:, 4] /= 3
  np.testing.assert_allclose(npy(amps), expected, rtol=1e-6)
  rng = np.random.default_rng(0)
  a, d, f = rng.uniform(0, 1, (2, 9, 1)), rng.uniform(0, 1, (2, 9, 12)), rng.uniform(100, 1500, (2, 9, 1))
  amps, freqs = ddsp.core.harmonic_to_sinusoidal(dev(a), dev(d), dev(f))
  ta, tf_ = T.harmonic_to_sinusoidal(a.astype(np.float32), d.astype(np.float32), f.astype(np.float32))
  parity_check(npy(amps), ta, 4e-6, 'harmonic_to_sinusoidal amplitudes')
  np.testing.assert_allclose(npy(freqs), tf_, rtol=1e-6)


# ---- 2. the scale functions against fp64 truth ---------------------------------------------------------------------------
SCALE_CASES = {
    'sigmoid_d1': ('sigmoid', 1, {}), 'sigmoid_d10': ('sigmoid', 10, {}), 'sigmoid_d64': ('sigmoid', 64, {}),
    'sigmoid_d4_range': ('sigmoid', 4, dict(hz_min=30.0, hz_max=12000.0)),
    'softmax_d1': ('softmax', 1, {}), 'softmax_d64': ('softmax', 64, {}), 'softmax_d7_range': ('softmax', 7, dict(hz_min=40.0, hz_max=4000.0)),
}


def scale_fns(ddsp, kind):
  return ((ddsp.core.frequencies_sigmoid, T.frequencies_sigmoid) if kind == 'sigmoid' else
          (ddsp.core.frequencies_softmax, T.frequencies_softmax))


@pytest.mark.parametrize('case', sorted(SCALE_CASES))
@pytest.mark.parametrize('four_d', [False, True])
def test_frequency_scale_functions_vs_truth_forward_and_backward(ddsp, case, four_d):
  kind, depth, kw = SCALE_CASES[case]
  ours, truth = scale_fns(ddsp, kind)
  rng = np.random.default_rng(depth)
  x = (3.0 * rng.standard_normal((2, 5, 6, depth))).astype(np.float32)
  xin = dev(x if four_d else x.reshape(2, 5, 6 * depth), grad=True)
  out = ours(xin, depth=depth, **kw)
  hz, dx = truth(x, depth, grad=True, **kw)
  assert tuple(out.shape) == (2, 5, 6)
  parity_check(npy(out) / hz, np.ones_like(hz), C_CTL, 'frequencies_%s relative' % case)
  g = rng.standard_normal(hz.shape).astype(np.float32)
  out.backward(dev(g))
  want = (g[..., None].astype(np.float64) * dx).reshape(xin.shape)
  parity_check(npy(xin.grad), want, C_GRAD * np.abs(want).max(), 'frequencies_%s gradient' % case)


# ---- 3. synthesis against fp64 truth ----------------------------------------------------------------------------------------
FWD_CASES = {
    # name: (B, F, K, N, sample_rate, method, f_lo, f_hi)
    'shipped_f1000_k100': (2, 1000, 100, 64000, 16000, 'window', 20.0, None),
    'hop100': (2, 160, 20, 16000, 16000, 'window', 20.0, None),
    'hop37_linear': (2, 100, 7, 3700, 16000, 'linear', 20.0, None),
    'hop2048': (2, 8, 16, 16384, 16000, 'window', 20.0, None),
    'hop2048_top_octave': (1, 4, 3, 8192, 16000, 'window', 4000.0, None),
    'one_frame': (2, 1, 5, 1600, 16000, 'linear', 20.0, None),
    'k1': (2, 25, 1, 1600, 16000, 'window', 20.0, None),
    'k257': (1, 25, 257, 1600, 16000, 'window', 20.0, None),
    'sr48k': (2, 100, 30, 9600, 48000, 'window', 20.0, None),
    'small': (2, 25, 10, 1600, 16000, 'window', 20.0, None),
    'small_linear': (2, 25, 10, 1600, 16000, 'linear', 20.0, None),
    'ragged_chunk': (1, 30, 4, 2730, 16000, 'window', 20.0, None),
}


@pytest.mark.parametrize('case', sorted(FWD_CASES))
def test_get_signal_vs_truth(ddsp, case):
  B, F, K, N, sr, method, f_lo, f_hi = FWD_CASES[case]
  amps, freqs = T.control_inputs(len(case) + K, B, F, K, sr, f_lo, f_hi)
  out = npy(controls_synth(ddsp, N, sr, method).get_signal(dev(amps), dev(freqs)))
  truth = T.get_signal(amps, freqs, N, sr, method)
  assert out.shape == (B, N)
  parity_check(out, truth, fwd_tol(amps, freqs, N, sr, method), 'Sinusoidal.get_signal ' + case)


def test_get_signal_from_0_hz_to_just_under_nyquist(ddsp):
  B, F, K, N, sr = 2, 50, 12, 3200, 16000
  rng = np.random.default_rng(5)
  amps = rng.uniform(0, 1, (B, F, K)).astype(np.float32)
  freqs = rng.uniform(0.0, sr / 2.0 - 1.0, (B, F, K)).astype(np.float32)
  freqs[:, :, 0] = 0.0
  freqs[:, :, 1] = np.float32(sr / 2.0 - 1.0)
  out = npy(controls_synth(ddsp, N, sr).get_signal(dev(amps), dev(freqs)))
  parity_check(out, T.get_signal(amps, freqs, N, sr), fwd_tol(amps, freqs, N, sr), 'Sinusoidal.get_signal 0 Hz .. Nyquist - 1')


RAW_CASES = {
    'sigmoid_default': (None, 1), 'sigmoid_d64': ('sigmoid', 64), 'softmax_d1': ('softmax', 1), 'softmax_d64': ('softmax', 64),
}


def raw_setup(ddsp, case, N, sr=16000):
  kind, depth = RAW_CASES[case]
  if kind is None:
    return ddsp.synths.Sinusoidal(n_samples=N, sample_rate=sr), T.frequencies_sigmoid, 1
  ours, truth = scale_fns(ddsp, kind)
  # hz_max above Nyquist: saturated network outputs land clearly beyond it and are masked at frame rate
  synth = ddsp.synths.Sinusoidal(n_samples=N, sample_rate=sr, freq_scale_fn=functools.partial(ours, depth=depth, hz_max=9000.0))
  return synth, functools.partial(truth, depth=depth, hz_max=9000.0), depth


@pytest.mark.parametrize('case', sorted(RAW_CASES))
def test_call_from_raw_inputs_vs_truth(ddsp, case):
  B, F, K, N, sr = 2, 25, 6, 1600, 16000
  synth, truth_fn, depth = raw_setup(ddsp, case, N, sr)
  rng = np.random.default_rng(depth + len(case))
  amps = rng.standard_normal((B, F, K)).astype(np.float32)
  freqs = (2.0 * rng.standard_normal((B, F, K * depth))).astype(np.float32)
  saturated = RAW_CASES[case][0] is not None
  if saturated:
    freqs[:, :, 0:depth] = 30.0 if RAW_CASES[case][0] == 'sigmoid' else np.linspace(-40.0, 40.0, depth) if depth > 1 else 0.0
  out = synth(dev(amps), dev(freqs), return_outputs_dict=True)
  ctl_a, ctl_f = npy(out['controls']['amplitudes']), npy(out['controls']['frequencies'])
  ta, tf_ = T.get_controls(amps, freqs, sr, True, truth_fn)
  if saturated and not (RAW_CASES[case][0] == 'softmax' and depth == 1):          # (softmax of one value sits at hz_min)
    assert np.all(tf_[:, :, 0] > 8500.0) and np.all(ctl_a[:, :, 0] == 0.0) and np.all(ta[:, :, 0] == 0.0)
  parity_check(ctl_f / tf_, np.ones_like(tf_), C_CTL, 'Sinusoidal controls frequencies (relative) ' + case)
  parity_check(ctl_a, ta, C_CTL * 2.0, 'Sinusoidal controls amplitudes ' + case)
  truth = T.get_signal(ctl_a, ctl_f, N, sr)
  parity_check(npy(out['signal']), truth, fwd_tol(ctl_a, ctl_f, N, sr), 'Sinusoidal() at its own controls ' + case)
  assert torch.equal(synth(dev(amps), dev(freqs)), out['signal'])
  two = synth.get_controls(dev(amps), dev(freqs))
  assert torch.equal(two['amplitudes'], out['controls']['amplitudes']) and torch.equal(two['frequencies'], out['controls']['frequencies'])
  assert torch.equal(synth.get_signal(**two), out['signal'])


def test_opaque_scale_function_runs_as_given(ddsp):
  B, F, K, N, depth = 2, 25, 4, 1600, 3
  rng = np.random.default_rng(9)
  amps = rng.standard_normal((B, F, K)).astype(np.float32)
  freqs = rng.standard_normal((B, F, K * depth)).astype(np.float32)
  closure = ddsp.synths.Sinusoidal(n_samples=N, freq_scale_fn=lambda x: ddsp.core.frequencies_sigmoid(x, depth=depth))
  fused = ddsp.synths.Sinusoidal(n_samples=N, freq_scale_fn=functools.partial(ddsp.core.frequencies_sigmoid, depth=depth))
  assert closure._freq_spec() is None and fused._freq_spec() is not None
  assert torch.equal(closure(dev(amps), dev(freqs)), fused(dev(amps), dev(freqs)))
  a, f = dev(amps, True), dev(freqs, True)
  closure(a, f).sum().backward()
  a2, f2 = dev(amps, True), dev(freqs, True)
  fused(a2, f2).sum().backward()
  assert torch.equal(a.grad, a2.grad) and torch.equal(f.grad, f2.grad)


# ---- 4. goldens, cross-checks ---------------------------------------------------------------------------------------------
GOLDEN_CLASS = ['sinusoidal_class_default_f25_k8', 'sinusoidal_class_softmax_d16_linear', 'sinusoidal_controls_f50_k6']


@pytest.mark.parametrize('name', GOLDEN_CLASS)
def test_class_vs_reference_golden(ddsp, name):
  z = load_golden(name)
  kind, depth = str(z['freq_fn']), int(z['depth'])
  fn = None if kind == 'none' else functools.partial(scale_fns(ddsp, kind)[0], depth=depth, hz_max=float(z['hz_max']))
  synth = ddsp.synths.Sinusoidal(n_samples=int(z['n_samples']), sample_rate=int(z['sample_rate']),
                                 amp_scale_fn=ddsp.core.exp_sigmoid if int(z['amp_scale']) else None, freq_scale_fn=fn,
                                 amp_resample_method=str(z['method']))
  parity_check(npy(synth(dev(z['amplitudes']), dev(z['frequencies']))), z['audio'], GOLDEN_TOL, 'golden ' + name)


def test_scale_functions_and_conversion_vs_reference_golden(ddsp):
  z = load_golden('sinusoidal_scale_functions')
  for kind in ('sigmoid', 'softmax'):
    for depth in (1, 8):
      out = npy(scale_fns(ddsp, kind)[0](dev(z['x_d%d' % depth]), depth=depth))
      want = z['%s_d%d' % (kind, depth)]
      parity_check(out / want, np.ones_like(want), 2e-5, 'golden frequencies_%s depth %d (relative)' % (kind, depth))
  amps, freqs = ddsp.core.harmonic_to_sinusoidal(dev(z['harm_amp']), dev(z['harm_dist']), dev(z['f0_hz']))
  parity_check(npy(amps), z['sin_amps'], 2e-6, 'golden harmonic_to_sinusoidal amplitudes')
  np.testing.assert_allclose(npy(freqs), z['sin_freqs'], rtol=1e-6)


def test_sinusoidal_of_harmonic_controls_equals_harmonic(ddsp):
  B, F, K, N, sr = 2, 50, 20, 3200, 16000
  rng = np.random.default_rng(11)
  amp = rng.uniform(0.2, 1.0, (B, F, 1)).astype(np.float32)
  dist = rng.uniform(0.0, 1.0, (B, F, K)).astype(np.float32)
  dist /= dist.sum(-1, keepdims=True)
  f0 = np.exp(rng.uniform(np.log(80.0), np.log(600.0), (B, F, 1))).astype(np.float32)       # 20 harmonics cross Nyquist above 400 Hz
  f0 += (np.abs(f0 * np.arange(1, K + 1) - sr / 2.0).min(-1, keepdims=True) < 1.0) * 3.0      # ... by at least 1 Hz
  harmonic = ddsp.synths.Harmonic(n_samples=N, sample_rate=sr, scale_fn=None, normalize_below_nyquist=True)
  harmonic.kernel = 'direct'
  ctl = harmonic.get_controls(dev(amp), dev(dist), dev(f0))
  want = npy(harmonic.get_signal(**ctl))
  a, f = ddsp.core.harmonic_to_sinusoidal(ctl['amplitudes'], ctl['harmonic_distribution'], ctl['f0_hz'], sr)
  out = npy(controls_synth(ddsp, N, sr).get_signal(a, f))
  parity_check(out, want, 2.0 * fwd_tol(npy(a), npy(f), N, sr), 'Sinusoidal(harmonic_to_sinusoidal) vs Harmonic')


CHAIN_CASES = {'window': (2, 25, 6, 1600, 'window'), 'linear_hop37': (2, 20, 5, 740, 'linear')}


@pytest.mark.parametrize('case', sorted(CHAIN_CASES))
def test_fused_path_vs_materialised_chain(ddsp, case):
  B, F, K, N, method = CHAIN_CASES[case]
  amps, freqs = T.control_inputs(3, B, F, K)
  synth = controls_synth(ddsp, N, 16000, method)
  a, f = dev(amps, True), dev(freqs, True)
  fused = synth.get_signal(a, f)
  g = dev(np.random.default_rng(1).standard_normal((B, N)))
  fused.backward(g)
  a2, f2 = dev(amps, True), dev(freqs, True)
  chain = ddsp.synths._SinusoidalChainFunction.apply(a2, f2, synth, 0, 1, 0.0, 0.0, False)[0]
  chain.backward(g)
  tol = fwd_tol(amps, freqs, N, 16000, method)
  parity_check(npy(fused), npy(chain), 2.0 * tol, 'fused vs chain audio ' + case)
  parity_check(npy(a.grad), npy(a2.grad), 2.0 * C_GRAD * float(a2.grad.abs().max()), 'fused vs chain dL/dA ' + case)
  parity_check(npy(f.grad), npy(f2.grad), 2.0 * C_GRAD * float(f2.grad.abs().max()), 'fused vs chain dL/df ' + case)


@pytest.mark.parametrize('case', ['cubic', 'nearest', 'ragged_linear', 'two_frame_grids'])
def test_chain_covers_the_rest_of_the_argument_space(ddsp, case):
  import oracle.ddsp_oracle as O
  method, N, Fa, Ff = {'cubic': ('cubic', 1600, 25, 25), 'nearest': ('nearest', 1600, 25, 25),
                       'ragged_linear': ('linear', 1000, 30, 30), 'two_frame_grids': ('linear', 1200, 10, 24)}[case]
  rng = np.random.default_rng(2)
  amps = rng.uniform(0, 1, (2, Fa, 4)).astype(np.float32)
  freqs = np.exp(rng.uniform(np.log(50.0), np.log(3000.0), (2, Ff, 4))).astype(np.float32)
  synth = controls_synth(ddsp, N, 16000, method)
  a, f = dev(amps, True), dev(freqs, True)
  out = synth(a, f)
  want = O.oscillator_bank(O.resample(freqs, N, dtype=np.float64), O.resample(amps, N, method, dtype=np.float64), 16000)
  parity_check(npy(out), want, C_FWD * max(1.0, float(amps.sum(-1).max())) + 2e-4, 'chain ' + case)   # (fp32 resize positions)
  out.sum().backward()
  assert a.grad.shape == a.shape and f.grad.shape == f.shape and bool(torch.isfinite(f.grad).all())


# ---- 5. the knife edge: a frame that crosses Nyquist --------------------------------------------------------------------------
def test_audio_rate_nyquist_mask_takes_the_references_side_sample_by_sample(ddsp):
  hop, sr = 64, 16000
  freqs = np.array([7000.0, 9000.0, 9000.0, 7000.0, 7000.0], np.float32)[None, :, None]      # exact in fp32: r / 64 * 2000
  amps = np.ones((1, 5, 1), np.float32)
  N = 5 * hop
  synth = controls_synth(ddsp, N, sr)
  out = npy(synth.get_signal(dev(amps), dev(freqs)))[0]
  truth = T.get_signal(amps, freqs, N, sr)[0]
  f_env = T.envelopes(amps, freqs, N)[1][0, :, 0]
  masked = f_env >= sr / 2.0
  assert masked[:32].sum() == 0 and masked[32:64].all()            # 7000 -> 9000 reaches 8000 at r = 32: masked from there on
  assert masked[64:128].all() and masked[128:161].all() and not masked[161:].any()     # 9000 -> 7000: r = 32 is 8000, still masked
  assert np.all(out[masked] == 0.0)
  assert np.count_nonzero(out[~masked]) > 0.9 * (~masked).sum()
  parity_check(out, truth, C_FWD, 'Nyquist knife edge')
  # no gradient through masked samples
  a, f = dev(amps, True), dev(freqs, True)
  g = np.zeros((1, N), np.float32)
  g[0, masked] = 1.0
  synth.get_signal(a, f).backward(dev(g))
  assert float(a.grad.abs().max()) == 0.0 and float(f.grad.abs().max()) == 0.0


# ---- 6. gradients ------------------------------------------------------------------------------------------------------------
GRAD_CASES = {
    'small': (2, 25, 6, 1600, 'window'), 'linear_hop37': (2, 20, 5, 740, 'linear'), 'one_frame': (1, 1, 3, 400, 'linear'),
    'hop2048': (1, 3, 4, 6144, 'window'), 'k70_two_blocks': (1, 8, 70, 512, 'window'),
}


@pytest.mark.parametrize('scale', [1e-6, 1.0, 1e6])
@pytest.mark.parametrize('case', sorted(GRAD_CASES))
def test_get_signal_gradients_vs_truth(ddsp, case, scale):
  B, F, K, N, method = GRAD_CASES[case]
  amps, freqs = T.control_inputs(len(case), B, F, K, f_hi=3000.0)
  g = (np.random.default_rng(4).standard_normal((B, N)) * scale).astype(np.float32)
  a, f = dev(amps, True), dev(freqs, True)
  controls_synth(ddsp, N, 16000, method).get_signal(a, f).backward(dev(g))
  ga, gf = T.get_signal_backward(amps, freqs, g, N, 16000, method)
  parity_check(npy(a.grad), ga, C_GRAD * np.abs(ga).max(), 'dL/d amplitudes %s x%g' % (case, scale))
  parity_check(npy(f.grad), gf, C_GRAD * np.abs(gf).max(), 'dL/d frequencies %s x%g' % (case, scale))


@pytest.mark.parametrize('case', sorted(RAW_CASES))
def test_call_gradients_through_the_scale_functions_vs_truth(ddsp, case):
  B, F, K, N, sr = 2, 25, 5, 1600, 16000
  synth, truth_fn, depth = raw_setup(ddsp, case, N, sr)
  rng = np.random.default_rng(depth)
  amps = rng.standard_normal((B, F, K)).astype(np.float32)
  freqs = (1.5 * rng.standard_normal((B, F, K * depth)) - (0.0 if depth > 1 else 1.0)).astype(np.float32)
  g = rng.standard_normal((B, N)).astype(np.float32)
  a, f = dev(amps, True), dev(freqs, True)
  out = synth(a, f, return_outputs_dict=True)
  out['signal'].backward(dev(g))
  # the synthesis' gradient at the fp32 controls the kernels ran on (as the forward comparison), the rest of the chain in fp64
  controls = (npy(out['controls']['amplitudes']), npy(out['controls']['frequencies']))
  ga, gf = T.sinusoidal_backward(amps, freqs, g, N, sr, 'window', True, freq_fn_grad=functools.partial(truth_fn, grad=True),
                                 controls=controls)
  parity_check(npy(a.grad), ga, C_GRAD * np.abs(ga).max(), 'dL/d raw amplitudes ' + case)
  parity_check(npy(f.grad), gf, C_GRAD * np.abs(gf).max(), 'dL/d raw frequencies ' + case)


# ---- 7. determinism, memory, DAG ----------------------------------------------------------------------------------------------
def test_bit_stable_forward_and_gradients(ddsp):
  B, F, K, N = 4, 25, 9, 1600
  rng = np.random.default_rng(8)
  amps = rng.standard_normal((B, F, K)).astype(np.float32)
  freqs = rng.standard_normal((B, F, K)).astype(np.float32)
  g = rng.standard_normal((B, N)).astype(np.float32)
  synth = ddsp.synths.Sinusoidal(n_samples=N)

  def run(rows):
    a, f = dev(amps[rows], True), dev(freqs[rows], True)
    out = synth(a, f)
    out.backward(dev(g[rows]))
    return out.detach(), a.grad, f.grad

  full, again = run(slice(0, 4)), run(slice(0, 4))
  alone, sub = run(slice(2, 3)), run(slice(1, 3))
  for x, y in zip(full, again):
    assert torch.equal(x, y)
  for x, y, z in zip(full, alone, sub):
    assert torch.equal(x[2:3], y) and torch.equal(x[1:3], z)


def test_peak_memory_stays_below_one_envelope(ddsp):
  B, F, K, N = 8, 1000, 100, 64000
  rng = np.random.default_rng(0)
  a = dev(rng.standard_normal((B, F, K)), True)
  f = dev(rng.standard_normal((B, F, K)), True)
  g = dev(rng.standard_normal((B, N)))
  synth = ddsp.synths.Sinusoidal(n_samples=N)
  synth(a, f).backward(g)                                              # workspaces exist from here on: they count
  a.grad = f.grad = None
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  out = synth(a, f)
  out.backward(g)
  torch.cuda.synchronize()
  extra = torch.cuda.max_memory_allocated() - before
  in_out = 4 * (B * N + 2 * B * F * K)                                 # the audio and the two gradients
  assert extra - in_out < 4 * B * N * K, 'forward + backward allocated %d bytes beyond inputs and outputs' % (extra - in_out)
  ws = synth._ws.get(0, a.device).numel() + synth._ws_bwd.get(0, a.device).numel()
  assert ws < 4 * B * N * K, 'workspaces hold %d bytes' % ws


def test_processor_group_with_sinusoidal_runs_and_differentiates(ddsp):
  N, F = 1600, 25
  sin = ddsp.synths.Sinusoidal(n_samples=N)
  noise = ddsp.synths.FilteredNoise(n_samples=N)
  add = ddsp.processors.Add()
  dag = [(sin, ['amps', 'freqs']), (noise, ['magnitudes']), (add, ['filtered_noise/signal', 'sinusoidal/signal'])]
  group = ddsp.processors.ProcessorGroup(dag=dag)
  rng = np.random.default_rng(3)
  feats = {'amps': dev(rng.standard_normal((2, F, 8)), True), 'freqs': dev(rng.standard_normal((2, F, 8)), True),
           'magnitudes': dev(rng.standard_normal((2, F, 65)), True)}
  out = group(feats)
  assert tuple(out.shape) == (2, N)
  out.square().sum().backward()
  for key in feats:
    assert feats[key].grad is not None and bool(torch.isfinite(feats[key].grad).all()) and float(feats[key].grad.abs().max()) > 0
